"""The wide gene emitter (hmm_gene_emissions_wide + hmm_gene_emissions_grad_wide) against the torch-op path
(GenePredHMMEmitter.forward, can_fuse forced False), same process, same inputs: the 43-, 71- and 253-state models
(3 and 5 copies shared, 18 copies unshared) at b L = 6.4e5 (b = 64, L = 10 000).

  python tools/experiments/emitter_wide_time.py

Prints per model
  * the wide forward alone (median of 7 after a warm-up, HIP events) and its bytes/s of in + out
    (4 (s + 5) bytes read and 4 q written per position);
  * the inference forward through the module, fused against torch ops: milliseconds and peak bytes;
  * one forward + backward of the fused node with loss = (E G).sum() against autograd through forward(): milliseconds
    and peak bytes (torch.cuda.max_memory_allocated above what was allocated before the step); the torch path is
    skipped where it runs out of memory;
and, on the 29-state model, hmm_gene_emissions_wide next to hmm_gene_emissions."""
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
B_, L_, S_ = 64, 10000, 15


def emitter(copies, shared):
    em = GenePredHMMEmitter(**CODONS, num_copies=copies, share_intron_parameters=shared)
    em.build((1, 1, 1, S_))
    with torch.no_grad():
        em.emission_kernel.copy_(torch.randn(em.emission_kernel.shape))
    return em.to(dev)


def inputs(q):
    g = torch.Generator(device=dev).manual_seed(q)
    cls = torch.softmax(2 * torch.randn((1, B_, L_, S_), generator=g, device=dev), -1)
    nuc = torch.nn.functional.one_hot(torch.randint(0, 5, (1, B_, L_), generator=g, device=dev), 5).float()
    return torch.cat([cls, nuc], -1).contiguous(), torch.randn((1, B_, L_, q), generator=g, device=dev)


def event_ms(fn, reps=7):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def wall(fn, reps=5):
    fn()
    torch.cuda.synchronize()
    ts, peak = [], 0
    for _ in range(reps):
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
        peak = max(peak, torch.cuda.max_memory_allocated() - base)
        del out
    return 1e3 * float(np.median(ts)), peak


def engine_args(em, x):
    row, cod = em.state_tables(dev)
    with torch.no_grad():
        B = em.make_B()[0].contiguous()
    return x[0], B, row, em.codon_probs.to(dev, torch.float32).contiguous(), cod


def step(em, x, G, fused):
    xs = x.detach().requires_grad_(True)
    em.zero_grad(set_to_none=True)
    em.recurrent_init()
    E = em.forward_fused_trainable(xs, training=True) if fused else em(xs, training=True)
    (E * G).sum().backward()
    return xs.grad, em.emission_kernel.grad


def infer(em, x, fused):
    with torch.no_grad():
        em.recurrent_init()
        return em.forward_fused(x) if fused else em(x)


def versus(label, fused, torch_ops):
    tf, pf = wall(fused)
    print("  %s fused: %.2f ms, peak %.1f MiB" % (label, tf, pf / 2**20), flush=True)
    try:
        tt, pt = wall(torch_ops)
        print("  %s torch: %.2f ms, peak %.1f MiB  -> fused is %.1fx faster, %.1fx smaller"
              % (label, tt, pt / 2**20, tt / tf, pt / pf), flush=True)
    except torch.cuda.OutOfMemoryError:
        print("  %s torch: out of memory" % label, flush=True)
    torch.cuda.empty_cache()


def main():
    n = B_ * L_
    for copies, shared in ((3, True), (5, True), (18, False)):
        em = emitter(copies, shared)
        q = em.num_states
        x, G = inputs(q)
        assert em.can_fuse(x) and em.fused_route() == "wide"
        args = engine_args(em, x)
        t = event_ms(lambda: engine.gene_emissions_wide(*args))
        print("%d states (%d rows), b L = %d: wide forward %.3f ms, %.2f TB/s of in + out"
              % (q, em.kernel_rows(), n, t, 4 * n * (S_ + 5 + q) / t / 1e9), flush=True)
        for name, want in (("dx + dB", {}), ("dx only", dict(want_dB=False)), ("dB only", dict(want_dx=False))):
            t = event_ms(lambda: engine.gene_emissions_grad_wide(*args, G[0], add=1e-7, **want))
            print("  wide backward alone, %s: %.3f ms" % (name, t), flush=True)
        versus("inference forward", lambda: infer(em, x, True), lambda: infer(em, x, False))
        versus("forward + backward", lambda: step(em, x, G, True), lambda: step(em, x, G, False))
        del x, G, args
        torch.cuda.empty_cache()
    em = emitter(2, True)
    x, _ = inputs(29)
    args = engine_args(em, x)
    tn = event_ms(lambda: engine.gene_emissions(*args))
    tw = event_ms(lambda: engine.gene_emissions_wide(*args))
    byts = 4 * n * (S_ + 5 + 29)
    print("29 states: hmm_gene_emissions %.3f ms (%.2f TB/s), hmm_gene_emissions_wide %.3f ms (%.2f TB/s)"
          % (tn, byts / tn / 1e9, tw, byts / tw / 1e9), flush=True)


if __name__ == "__main__":
    main()
