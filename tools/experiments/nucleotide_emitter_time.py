"""Trainable nucleotide factor (trainable_nucleotides_at_exons=True): the fused paths (hmm_gene_emissions[_wide], then
hmm_nucleotide_emissions; training: autograd.GeneEmissions and autograd.NucleotideEmissions) against the torch-op path of
the same model (GenePredHMMEmitter.forward, what this model ran before the kernels existed), same process, same inputs.

  python tools/experiments/nucleotide_emitter_time.py [--headline]

Prints, for the 15-, 29- and 43-state models at b L = 6.4e5 (b = 64, L = 10 000; with --headline also b = 1024,
L = 100 000, every step that runs out of memory reported as such), each a median of 7 after a warm-up with a device
synchronise inside the timed window:
  * forward_fused (inference) and forward() under no_grad, milliseconds and peak bytes allocated;
  * forward + backward with loss = (E G).sum() through forward_fused_trainable and through forward(), training=True,
    milliseconds and peak bytes;
  * hmm_nucleotide_emissions(multiply=1) and hmm_nucleotide_emissions_grad (both outputs) alone, with the bytes they
    move: E read and written (backward: dE read, dE_in written, E_in read on the exon states) plus the five nucleotide
    floats of every position (whole rows of x come through the cache hierarchy; only the 20 bytes count here)."""
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


def inputs(b, L, q):
    g = torch.Generator(device=dev).manual_seed(b + L + q)
    cls = torch.softmax(2 * torch.randn((1, b, L, S), generator=g, device=dev), -1)
    nuc = torch.nn.functional.one_hot(torch.randint(0, 5, (1, b, L), generator=g, device=dev), 5).float()
    return torch.cat([cls, nuc], -1).contiguous(), torch.randn((1, b, L, q), generator=g, device=dev)


def timed(fn, reps=7):
    """-> (median milliseconds, peak bytes allocated above the state before the call)."""
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


def train_step(em, x, G, fused):
    xs = x.detach().requires_grad_(True)
    em.zero_grad(set_to_none=True)
    em.recurrent_init()
    E = em.forward_fused_trainable(xs, training=True) if fused else em(xs, training=True)
    (E * G).sum().backward()
    return xs.grad, em.emission_kernel.grad, em.nuc_emission_kernel.grad


def infer(em, x, fused):
    with torch.no_grad():
        em.recurrent_init()
        return em.forward_fused(x) if fused else em(x)


def pair(tag, fused_fn, torch_fn):
    try:
        tf, pf = timed(fused_fn)
        print("%s fused: %.3f ms, peak %.1f MiB" % (tag, tf, pf / 2**20), flush=True)
    except torch.cuda.OutOfMemoryError:
        print("%s fused: out of memory" % tag, flush=True)
        return
    finally:
        torch.cuda.empty_cache()
    try:
        tt, pt = timed(torch_fn)
        print("%s torch ops: %.3f ms, peak %.1f MiB  -> fused is %.2fx faster, %.1fx smaller"
              % (tag, tt, pt / 2**20, tt / tf, pt / max(pf, 1)), flush=True)
    except torch.cuda.OutOfMemoryError:
        print("%s torch ops: out of memory" % tag, flush=True)
    finally:
        torch.cuda.empty_cache()


def main():
    shapes = [(64, 10000)] + ([(1024, 100000)] if "--headline" in sys.argv else [])
    for b, L in shapes:
        for copies in (1, 2, 3):
            em = GenePredHMMEmitter(**CODONS, num_copies=copies, trainable_nucleotides_at_exons=True)
            em.build((1, 1, 1, S))
            with torch.no_grad():
                em.emission_kernel.copy_(torch.randn(em.emission_kernel.shape))
                em.nuc_emission_kernel.copy_(torch.randn(em.nuc_emission_kernel.shape))
            em = em.to(dev)
            q = em.num_states
            tag = "q=%d b=%d L=%d" % (q, b, L)
            try:
                x, G = inputs(b, L, q)
            except torch.cuda.OutOfMemoryError:
                print("%s: inputs do not fit" % tag, flush=True)
                torch.cuda.empty_cache()
                continue
            pair(tag + " inference", lambda: infer(em, x, True), lambda: infer(em, x, False))
            pair(tag + " forward + backward", lambda: train_step(em, x, G, True), lambda: train_step(em, x, G, False))
            try:
                with torch.no_grad():
                    P = em.get_nucleotide_probs()[0].contiguous()
                tab = em.nucleotide_table(dev)
                E = 0.5 + torch.rand((b, L, q), device=dev)
                dE = G[0].contiguous()
                n = b * L
                t, _ = timed(lambda: engine.nucleotide_emissions(x[0], S, P, tab, E=E))
                moved = n * (8 * q + 20)
                print("%s hmm_nucleotide_emissions alone: %.3f ms, %.1f MB moved, %.2f TB/s"
                      % (tag, t, moved / 1e6, moved / t / 1e9), flush=True)
                t, _ = timed(lambda: engine.nucleotide_emissions_grad(x[0], S, P, tab, dE, E_in=E))
                moved = n * (8 * q + 12 * copies + 20)         # E_in is read on the 3 c exon states only
                print("%s hmm_nucleotide_emissions_grad alone: %.3f ms, %.1f MB moved, %.2f TB/s"
                      % (tag, t, moved / 1e6, moved / t / 1e9), flush=True)
                del E, dE
            except torch.cuda.OutOfMemoryError:
                print("%s kernels alone: out of memory" % tag, flush=True)
            del x, G
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
