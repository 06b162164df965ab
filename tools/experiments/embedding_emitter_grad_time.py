"""Embedding emitter forward + backward: the fused nodes (autograd.GeneEmissions, autograd.EmbeddingEmissions:
hmm_embedding_emissions + hmm_embedding_emissions_grad) against the torch-op path of the same tree
(GenePredHMMEmitter.forward under autograd, what fused_training=False runs), same process, same inputs, 15-state
gene model, training=True.

  python tools/experiments/embedding_emitter_grad_time.py

Prints, per d in {32, 64, 256} at b L = 6.4e5 (b = 64, L = 10 000; the torch path is skipped where it runs out of
memory), the milliseconds of one forward + backward with loss = (E G).sum() (median of 5 after a warm-up, a device
synchronise inside the timed window) and the peak bytes allocated during it (torch.cuda.max_memory_allocated above
what was allocated before the step), then the time of the backward call alone with all outputs and with each
output group alone."""
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
S = 15


def inputs(b, L, d):
    g = torch.Generator(device=dev).manual_seed(b + L + d)
    cls = torch.softmax(2 * torch.randn((1, b, L, S), generator=g, device=dev), -1)
    emb = torch.randn((1, b, L, d), generator=g, device=dev)
    nuc = torch.nn.functional.one_hot(torch.randint(0, 5, (1, b, L), generator=g, device=dev), 5).float()
    return torch.cat([cls, emb, nuc], -1).contiguous(), torch.randn((1, b, L, 15), generator=g, device=dev)


def step(em, x, G, fused):
    xs = x.detach().requires_grad_(True)
    em.zero_grad(set_to_none=True)
    em.recurrent_init()
    E = em.forward_fused_trainable(xs, training=True) if fused else em(xs, training=True)
    (E * G).sum().backward()
    return xs.grad, em.emission_kernel.grad, em.embedding_emission_kernel.grad


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


def backward_alone(em, x, G, E_in, reps=5, **want):
    d = em.embedding_dim
    row, _ = em.state_tables(dev)
    args = (x[0], S, d, *em.embedding_tables(dev), row, G[0].contiguous())
    kw = dict(E_in=E_in, inv_temperature=1.0 / float(em.temperature), add=1e-10, **want)
    engine.embedding_emissions_grad(*args, **kw)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        engine.embedding_emissions_grad(*args, **kw)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts))


def main():
    b, L = 64, 10000
    for d in (32, 64, 256):
        em = GenePredHMMEmitter(**CODONS, emit_embeddings=True, embedding_dim=d, temperature=float(d))
        em.build((1, 1, 1, S))
        with torch.no_grad():
            em.emission_kernel.copy_(torch.randn(em.emission_kernel.shape))
            ker = torch.randn(em.embedding_emission_kernel.shape)
            ker[..., d:] = 0.3 + 0.3 * ker[..., d:]
            em.embedding_emission_kernel.copy_(ker)
        em = em.to(dev)
        x, G = inputs(b, L, d)
        tf, pf = measure(em, x, G, True)
        print("d=%d b=%d L=%d fused: %.2f ms, peak %.1f MiB (x is %.1f MiB)" % (d, b, L, tf, pf / 2**20, x.numel() * 4 / 2**20),
              flush=True)
        try:
            tt, pt = measure(em, x, G, False)
            print("d=%d b=%d L=%d torch: %.2f ms, peak %.1f MiB  -> fused is %.2fx faster, %.1fx smaller"
                  % (d, b, L, tt, pt / 2**20, tt / tf, pt / pf), flush=True)
        except torch.cuda.OutOfMemoryError:
            print("d=%d b=%d L=%d torch: out of memory" % (d, b, L), flush=True)
        torch.cuda.empty_cache()
        E_in = 0.5 + torch.rand((b, L, 15), device=dev)
        off = dict(want_dE_in=False, want_demb=False, want_tables=False)
        for name, want in (("all outputs", {}), ("dE_in only", dict(off, want_dE_in=True)),
                           ("demb only", dict(off, want_demb=True)), ("tables only", dict(off, want_tables=True))):
            t = backward_alone(em, x, G, E_in, **want)
            print("d=%d b=%d L=%d backward alone, %s: %.3f ms" % (d, b, L, name, t), flush=True)
        del x, G, E_in
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
