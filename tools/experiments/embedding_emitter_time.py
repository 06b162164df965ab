#!/usr/bin/env python3
"""Time the fused inference path of an embedding emitter (GenePredHMMEmitter.forward_fused: hmm_gene_emissions +
hmm_embedding_emissions) against forward() (torch ops) on the same device, and the embedding kernel alone.

15-state model, b*L about 6.4e5, d in {32, 64, 256}.  Device events around each call, warm-up first, several
repetitions, the median reported.  Bytes of the multiply pass: 4 * (b*L) * (d + 2q) (embedding columns read once,
E read and written once).  One JSON line per d.

    python tools/experiments/embedding_emitter_time.py [--b 64 --L 10000 --reps 20 --warmup 3]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from hmm_layer_amd import engine                                           # noqa: E402
from hmm_layer_amd.gene_pred_hmm_emitter import GenePredHMMEmitter         # noqa: E402

CODONS = dict(start_codons=[("ATG", 1.)], stop_codons=[("TAG", .34), ("TAA", .33), ("TGA", .33)],
              intron_begin_pattern=[("NGT", .99), ("NGC", .005), ("NAT", .005)],
              intron_end_pattern=[("AGN", .99), ("ACN", .01)])


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        ms.append(t0.elapsed_time(t1))
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--b", type=int, default=64)
    ap.add_argument("--L", type=int, default=10000)
    ap.add_argument("--dims", type=int, nargs="+", default=[32, 64, 256])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device: nothing is timed on the CPU"
    dev = torch.device("cuda:0")
    b, L, s = args.b, args.L, 15
    for d in args.dims:
        g = torch.Generator().manual_seed(d)
        em = GenePredHMMEmitter(**CODONS, emit_embeddings=True, embedding_dim=d, temperature=float(d))
        em.build((1, b, L, s))
        em = em.to(dev)
        x = torch.cat([torch.softmax(2 * torch.randn((1, b, L, s), device=dev), -1),
                       torch.randn((1, b, L, d), device=dev),
                       torch.nn.functional.one_hot(torch.randint(0, 4, (1, b, L), device=dev), 5).float()], -1)
        q = em.num_states
        with torch.no_grad():
            em.recurrent_init()
            assert em.can_fuse(x)
            fused = em.forward_fused(x)
            torch_E = em(x)
            rel = float(((fused - torch_E).abs() / torch_E.abs().clamp_min(1e-30)).max())
            del torch_E
            mean, inv_std, log_norm = em.embedding_tables(dev)
            row, _ = em.state_tables(dev)
            E = fused[0].contiguous().clone()
            del fused

            def torch_path():
                em(x)

            def fused_path():
                em.forward_fused(x)

            def kernel_multiply():
                engine.embedding_emissions(x[0], s, d, mean, inv_std, log_norm, row, E=E, inv_temperature=1.0 / d)

            t_torch = timed(torch_path, args.reps, args.warmup)
            t_fused = timed(fused_path, args.reps, args.warmup)
            E.fill_(1.0)
            t_kernel = timed(kernel_multiply, args.reps, args.warmup)      # E decays towards 0: same work
        nbytes = 4 * b * L * (d + 2 * q)
        print(json.dumps({"d": d, "b": b, "L": L, "q": q, "reps": args.reps,
                          "torch_forward_ms": round(t_torch[0], 4), "torch_min_max_ms": [round(v, 4) for v in t_torch[1:]],
                          "fused_forward_ms": round(t_fused[0], 4), "fused_min_max_ms": [round(v, 4) for v in t_fused[1:]],
                          "embedding_kernel_ms": round(t_kernel[0], 4),
                          "embedding_kernel_min_max_ms": [round(v, 4) for v in t_kernel[1:]],
                          "multiply_pass_bytes": nbytes,
                          "embedding_kernel_TBps": round(nbytes / (t_kernel[0] * 1e-3) / 1e12, 4),
                          "fused_vs_torch_max_rel_diff": rel}), flush=True)
        del x, E
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
