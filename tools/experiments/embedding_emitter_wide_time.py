"""The wide embedding kernels (hmm_embedding_emissions_wide + hmm_embedding_emissions_grad_wide) against the torch-op
path (GenePredHMMEmitter.forward, what emit_embeddings=True ran for three and more copies before them), same process,
same inputs: the 43-, 71- and 253-state models (3 and 5 copies shared, 18 copies unshared) at d = 64,
b L = 6.4e5 (b = 64, L = 10 000).

  python tools/experiments/embedding_emitter_wide_time.py

Prints per model
  * the wide forward alone (multiplying into E; median of 7 after a warm-up, HIP events) and its VALU rate against
    the difference form's 3 operations per (position, row, column);
  * the backward call alone for all outputs / dE_in / demb / the tables;
  * one training step (forward + backward, training=True, loss = (E G).sum()) of the fused module path against
    autograd through forward(): milliseconds and peak bytes (torch.cuda.max_memory_allocated above what was allocated
    before the step); where the torch path runs out of memory, that is printed instead of a time;
and, on the 29-state model, hmm_embedding_emissions next to hmm_embedding_emissions_wide.
Every GPU step runs under a time limit of its own (an alarm that ends the process)."""
import contextlib
import os
import signal
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
B_, L_, S_, D_ = 64, 10000, 15, 64


@contextlib.contextmanager
def limit(seconds, what):
    def over(signum, frame):
        print("time limit of %d s passed in: %s" % (seconds, what), flush=True)
        os._exit(124)
    signal.signal(signal.SIGALRM, over)
    signal.alarm(seconds)
    try:
        yield
    finally:
        signal.alarm(0)


def emitter(copies, shared, fused):
    em = GenePredHMMEmitter(**CODONS, num_copies=copies, share_intron_parameters=shared, emit_embeddings=True,
                            embedding_dim=D_, temperature=float(D_), fused_training=fused)
    em.build((1, 1, 1, S_))
    g = torch.Generator().manual_seed(copies)
    with torch.no_grad():
        em.emission_kernel.copy_(torch.randn(em.emission_kernel.shape, generator=g))
        ker = torch.randn(em.embedding_emission_kernel.shape, generator=g)
        ker[..., D_:] = 0.3 + 0.3 * ker[..., D_:]
        em.embedding_emission_kernel.copy_(ker)
    return em.to(dev)


def inputs(q):
    g = torch.Generator(device=dev).manual_seed(q)
    cls = torch.softmax(2 * torch.randn((1, B_, L_, S_), generator=g, device=dev), -1)
    emb = torch.randn((1, B_, L_, D_), generator=g, device=dev)
    nuc = torch.nn.functional.one_hot(torch.randint(0, 5, (1, B_, L_), generator=g, device=dev), 5).float()
    return torch.cat([cls, emb, nuc], -1).contiguous(), torch.randn((1, B_, L_, q), generator=g, device=dev)


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


def step(em, x, G, fused):
    xs = x.detach().requires_grad_(True)
    em.zero_grad(set_to_none=True)
    em.recurrent_init()
    E = em.forward_fused_trainable(xs, training=True) if fused else em(xs, training=True)
    (E * G).sum().backward()
    return xs.grad, em.embedding_emission_kernel.grad


def kernel_times(em, x, G, label):
    """The forward (multiplying into E) and the backward call alone, through the wide pair."""
    n = B_ * L_
    row, _ = em.state_tables(dev)
    mean, inv_std, log_norm = em.embedding_tables(dev)
    args = (x[0], S_, D_, mean, inv_std, log_norm, row)
    E = torch.rand((B_, L_, row.numel()), device=dev) + 0.5
    rows = mean.shape[0]
    ops = 3.0 * n * rows * D_
    with limit(120, label + " forward"):
        t = event_ms(lambda: engine.embedding_emissions_wide(*args, E=E.clone(), inv_temperature=1.0 / D_))
        tc = event_ms(lambda: E.clone())
    print("%s: wide forward %.3f ms including a %.3f ms copy of E -> %.3f ms, %.1f T VALU op/s"
          % (label, t, tc, t - tc, ops / (t - tc) / 1e9), flush=True)
    for name, want in (("all", {}), ("dE_in", dict(want_demb=False, want_tables=False)),
                       ("demb", dict(want_dE_in=False, want_tables=False)),
                       ("tables", dict(want_dE_in=False, want_demb=False))):
        with limit(120, label + " backward " + name):
            t = event_ms(lambda: engine.embedding_emissions_grad_wide(*args, G[0], E_in=E, inv_temperature=1.0 / D_,
                                                                      add=1e-10, **want))
        print("  wide backward alone, %s: %.3f ms" % (name, t), flush=True)
    return args, E


def main():
    n = B_ * L_
    for copies, shared in ((3, True), (5, True), (18, False)):
        em = emitter(copies, shared, True)
        q = em.num_states
        x, G = inputs(q)
        assert em.can_fuse(x) and em.fused_routes() == ("wide", "mvn_wide")
        label = "%d states (%d rows), d = %d, b L = %d" % (q, em.kernel_rows(), D_, n)
        kernel_times(em, x, G, label)
        with limit(180, label + " fused step"):
            tf, pf = wall(lambda: step(em, x, G, True))
        print("  forward + backward fused: %.2f ms, peak %.1f MiB" % (tf, pf / 2**20), flush=True)
        try:
            with limit(300, label + " torch step"):
                tt, pt = wall(lambda: step(em, x, G, False), reps=3)
            print("  forward + backward torch ops: %.2f ms, peak %.1f MiB  -> fused is %.1fx faster, %.1fx smaller"
                  % (tt, pt / 2**20, tt / tf, pt / pf), flush=True)
        except torch.cuda.OutOfMemoryError:
            print("  forward + backward torch ops: out of memory", flush=True)
        del x, G
        em.zero_grad(set_to_none=True)
        torch.cuda.empty_cache()
    em = emitter(2, True, True)
    x, G = inputs(29)
    row, _ = em.state_tables(dev)
    args = (x[0], S_, D_, *em.embedding_tables(dev), row)
    E = torch.rand((B_, L_, 29), device=dev) + 0.5
    with limit(120, "29 states"):
        tc = event_ms(lambda: E.clone())
        tn = event_ms(lambda: engine.embedding_emissions(*args, E=E.clone(), inv_temperature=1.0 / D_)) - tc
        tw = event_ms(lambda: engine.embedding_emissions_wide(*args, E=E.clone(), inv_temperature=1.0 / D_)) - tc
    print("29 states (25 rows), d = %d: hmm_embedding_emissions %.3f ms, hmm_embedding_emissions_wide %.3f ms "
          "(copy of E, %.3f ms, subtracted)" % (D_, tn, tw, tc), flush=True)


if __name__ == "__main__":
    main()
