"""Emitter forward + backward: the fused node (hmm_gene_emissions + hmm_gene_emissions_grad) against the torch-op path
(GenePredHMMEmitter.forward under autograd), same process, same inputs, 15-state gene model.

  python tools/experiments/emitter_grad_time.py [--prof]

Prints, per shape (b = 64 and b = 256 at L = 9 999; the torch path is skipped where it runs out of memory), the
milliseconds of one forward + backward with loss = (E G).sum() (median of 5 after a warm-up) and the peak bytes
allocated during it (torch.cuda.max_memory_allocated above what was allocated before the step), then the time of
the backward call alone with both outputs, dx only and dB only.
--prof runs the fused path only, three steps at b = 64 (for rocprofv3 --kernel-trace --stats)."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from hmm_layer_amd import engine  # noqa: E402
from hmm_layer_amd.gene_pred_hmm_emitter import GenePredHMMEmitter  # noqa: E402

dev = torch.device("cuda:0")
CODONS = dict(start_codons=[("ATG", 1.)], stop_codons=[("TAG", .34), ("TAA", .33), ("TGA", .33)],
              intron_begin_pattern=[("NGT", .99), ("NGC", .005), ("NAT", .005)],
              intron_end_pattern=[("AGN", .99), ("ACN", .01)])


def inputs(b, L):
    g = torch.Generator(device=dev).manual_seed(b + L)
    cls = torch.softmax(2 * torch.randn((1, b, L, 15), generator=g, device=dev), -1)
    nuc = torch.nn.functional.one_hot(torch.randint(0, 5, (1, b, L), generator=g, device=dev), 5).float()
    return torch.cat([cls, nuc], -1).contiguous(), torch.randn((1, b, L, 15), generator=g, device=dev)


def step(em, x, G, fused):
    xs = x.detach().requires_grad_(True)
    em.zero_grad(set_to_none=True)
    em.recurrent_init()
    E = em.forward_fused_trainable(xs, training=True) if fused else em(xs, training=True)
    (E * G).sum().backward()
    return xs.grad, em.emission_kernel.grad


def measure(em, x, G, fused, reps=5):
    step(em, x, G, fused)
    torch.cuda.synchronize()
    ts, peak = [], 0
    for _ in range(reps):
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        t0 = time.perf_counter()
        out = step(em, x, G, fused)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
        peak = max(peak, torch.cuda.max_memory_allocated() - base)
        del out
    return 1e3 * float(np.median(ts)), peak


def backward_alone(em, x, G, reps=5, **want):
    row, cod = em.state_tables(dev)
    with torch.no_grad():
        B = em.make_B()[0].contiguous()
    args = (x[0], B, row, em.codon_probs.to(dev, torch.float32).contiguous(), cod, G[0].contiguous())
    engine.gene_emissions_grad(*args, add=1e-7, **want)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        engine.gene_emissions_grad(*args, add=1e-7, **want)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts))


def main():
    prof = "--prof" in sys.argv
    em = GenePredHMMEmitter(**CODONS)
    em.build((1, 1, 1, 15))
    with torch.no_grad():
        em.emission_kernel.copy_(torch.randn(em.emission_kernel.shape))
    em = em.to(dev)
    for b, L in ((64, 9999),) if prof else ((64, 9999), (256, 9999)):
        x, G = inputs(b, L)
        if prof:
            for _ in range(3):
                step(em, x, G, True)
            torch.cuda.synchronize()
            return
        tf, pf = measure(em, x, G, True)
        print("b=%d L=%d fused: %.2f ms, peak %.1f MiB (x is %.1f MiB)" % (b, L, tf, pf / 2**20, x.numel() * 4 / 2**20),
              flush=True)
        try:
            tt, pt = measure(em, x, G, False)
            print("b=%d L=%d torch: %.2f ms, peak %.1f MiB  -> fused is %.1fx faster, %.1fx smaller"
                  % (b, L, tt, pt / 2**20, tt / tf, pt / pf), flush=True)
        except torch.cuda.OutOfMemoryError:
            print("b=%d L=%d torch: out of memory" % (b, L), flush=True)
        torch.cuda.empty_cache()
        n = b * L
        for name, want in (("dx + dB", {}), ("dx only", dict(want_dB=False)), ("dB only", dict(want_dx=False))):
            t = backward_alone(em, x, G, **want)
            byts = 4 * n * (15 + (20 if want.get("want_dB", True) else 5) + (20 if want.get("want_dx", True) else 0))
            print("b=%d L=%d backward alone, %s: %.3f ms (%.0f GB/s of algorithmic traffic)"
                  % (b, L, name, t, byts / t / 1e6), flush=True)
        del x, G
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
