"""hmm_loglik_grad_large: per-sequence walk (OPT_GLARGE = 1) against per-position GEMMs (= 2).

  python tools/experiments/lg_large_time.py [--prof]

Prints the milliseconds of one call (median of 3 after a warm-up):
  * the crossover that sets the default route: walk against GEMMs at b = 1024, L = 200, q = 65 / 100 / 128
    (the walk's limit);
  * the five-copy gene model (71 states) at b = 1024 x L = 1e4 under both evaluations;
  * the config-5 shape, q = 1027 x b = 1024: time per position from L = 6 and L = 38, next to hmm_forward's
    (log-likelihood only) in the same run;
  * a whole layer training step (forward + backward) of the five-copy model at b = 32 x L = 9999.
--prof runs the first two only (for rocprofv3 --kernel-trace --stats: tools/prof_one.sh)."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from hmm_layer_amd import engine  # noqa: E402

dev = torch.device("cuda:0")


def timed(fn, reps=3):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts))


def grad_ms(route, A, pi, E, reps=3):
    with engine.option(engine.OPT_GLARGE, route):
        return timed(lambda: engine.loglik_grad_large(A, pi, E), reps)


def gene5():
    from hmm_layer_amd.gene_pred_hmm_transitioner import GenePredMultiHMMTransitioner
    tr = GenePredMultiHMMTransitioner(k=5, initial_exon_len=200, initial_intron_len=4500, initial_ir_len=10000)
    with torch.no_grad():
        return tr.make_A().to(dev).contiguous(), tr.make_initial_distribution().reshape(1, -1).to(dev).contiguous()


def E_of(b, L, q):
    g = torch.Generator(device=dev).manual_seed(b + L + q)
    return (torch.rand((1, b, L, q), generator=g, device=dev) * 0.9 + 0.05).contiguous()


def band(q, seed=0):
    rng = np.random.default_rng(seed)
    A = np.zeros((q, q))
    for d in range(4):
        A[np.arange(q), (np.arange(q) + d) % q] = rng.random(q) + 0.1
    A /= A.sum(-1, keepdims=True)
    pi = np.full(q, 1.0 / q)
    return torch.tensor(A, dtype=torch.float32, device=dev)[None], torch.tensor(pi, dtype=torch.float32, device=dev)[None]


def layer_step(b, L):
    from hmm_layer_amd.MsaHmmCell import HmmCell
    from hmm_layer_amd.MsaHMMLayer import MsaHmmLayer
    from hmm_layer_amd.gene_pred_hmm_emitter import GenePredHMMEmitter
    from hmm_layer_amd.gene_pred_hmm_transitioner import GenePredMultiHMMTransitioner
    codons = dict(start_codons=[("ATG", 1.)], stop_codons=[("TAG", .34), ("TAA", .33), ("TGA", .33)],
                  intron_begin_pattern=[("NGT", .99), ("NGC", .005), ("NAT", .005)],
                  intron_end_pattern=[("AGN", .99), ("ACN", .01)])
    g = torch.Generator().manual_seed(1)
    cls = torch.softmax(2 * torch.randn((1, b, L, 15), generator=g), -1)
    nuc = torch.nn.functional.one_hot(torch.randint(0, 4, (1, b, L), generator=g), 5).float()
    x = torch.cat([cls, nuc], -1).to(dev)
    em = GenePredHMMEmitter(**codons, num_copies=5)
    em.build((1, b, L, 15))
    tr = GenePredMultiHMMTransitioner(k=5, initial_exon_len=200, initial_intron_len=4500, initial_ir_len=10000)
    cell = HmmCell([71], 15, em, tr).to(dev)
    layer = MsaHmmLayer(cell, use_prior=False)
    layer.build(x.shape)

    def step():
        for p in cell.parameters():
            p.grad = None
        _, mean = layer(x, training=True)
        (-mean).backward()
    return step


def main():
    if "--prof" not in sys.argv:
        for q in (65, 100, 128):
            A, pi = band(q)
            E = E_of(1024, 200, q)
            print("crossover q=%d b=1024 L=200: walk %.2f ms  GEMMs %.2f ms" % (q, grad_ms(1, A, pi, E), grad_ms(2, A, pi, E)),
                  flush=True)
            del E
    A, pi = gene5()
    E = E_of(1024, 10000, 71)
    tw, tg = grad_ms(1, A, pi, E), grad_ms(2, A, pi, E, reps=1)
    print("gene k=5 q=71 b=1024 L=1e4: walk %.2f ms  GEMMs %.2f ms  (GEMMs / walk %.1fx)" % (tw, tg, tg / tw), flush=True)
    del E
    A, pi = band(1027)
    tf, tgr = {}, {}
    for L in (6, 38):
        E = E_of(1024, L, 1027)
        tf[L] = timed(lambda: engine.forward(A, pi, E, want_log_alpha=False))
        tgr[L] = grad_ms(0, A, pi, E)
        del E
    pf, pg = 1e3 * (tf[38] - tf[6]) / 32, 1e3 * (tgr[38] - tgr[6]) / 32
    print("config 5 q=1027 b=1024: forward %.1f us, gradient %.1f us per position (%.2fx)" % (pf, pg, pg / pf),
          flush=True)
    if "--prof" in sys.argv:
        return
    step = layer_step(32, 9999)
    print("gene k=5 layer training step b=32 L=9999: %.2f ms" % timed(step), flush=True)


if __name__ == "__main__":
    main()
