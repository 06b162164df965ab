"""hmm_viterbi_large: per-sequence walk (OPT_VLARGE = 1) against per-position tiles (= 2).

  python tools/experiments/vit_large_time.py [--quick | --prof]

Prints, per shape, the milliseconds of one call under each evaluation (median of 3 after a warm-up):
  * the crossover sweep that sets the default route (VL_Q_WALK): b = 1024, L = 200, band / sparse / dense models;
  * the five-copy gene model (71 states) at b = 1024 x L = 1e4;
  * the config-5 shape, q = 1027 x b = 1024: the tile path's time per position from L = 6 and L = 38.
--prof runs only the last two (for rocprofv3 --kernel-trace --stats: tools/prof_one.sh)."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from hmm_layer_amd import engine  # noqa: E402
from tests import viterbi_wide as vw  # noqa: E402

dev = torch.device("cuda:0")


def timed(route, logA, logpi, logE, reps=3):
    with engine.option(engine.OPT_VLARGE, route):
        engine.viterbi_large(logA, logpi, logE)
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            engine.viterbi_large(logA, logpi, logE)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts))


def model(q, kind, seed=0):
    logA, logpi = vw.random_model(np.random.default_rng(seed), q, kind)
    return torch.tensor(logA, device=dev)[None], torch.tensor(logpi, device=dev)[None]


def gene5():
    from hmm_layer_amd.gene_pred_hmm_transitioner import GenePredMultiHMMTransitioner
    tr = GenePredMultiHMMTransitioner(k=5, initial_exon_len=200, initial_intron_len=4500, initial_ir_len=10000)
    with torch.no_grad():
        return (torch.log(tr.make_A()).to(dev).contiguous(),
                torch.log(tr.make_initial_distribution().reshape(1, -1)).to(dev).contiguous())


def logE_of(b, L, q):
    g = torch.Generator(device=dev).manual_seed(b + L + q)
    return (-6 * torch.rand((1, b, L, q), generator=g, device=dev)).contiguous()


def main():
    quick = "--quick" in sys.argv
    qs = (65, 128, 256, 512, 1024) if quick else (65, 71, 128, 129, 192, 256, 344, 512, 1024)
    kinds = ("sparse", "dense") if quick else ("sparse", "band", "dense")
    if "--prof" in sys.argv:
        kinds = ()
    b, L = 1024, 200
    for kind in kinds:
        for q in qs:
            A, pi = model(q, kind)
            E = logE_of(b, L, q)
            # (the all-candidates walk above 256 states reads log A from memory every step: not timed)
            tw = timed(1, A, pi, E) if kind == "sparse" or q <= 256 else float("nan")
            print("crossover %-6s q=%4d b=%d L=%d: walk %8.2f ms  tiles %8.2f ms" % (
                kind, q, b, L, tw, timed(2, A, pi, E)), flush=True)
            del E
    A, pi = gene5()
    E = logE_of(1024, 10000, 71)
    tw, tt = timed(1, A, pi, E), timed(2, A, pi, E)
    print("gene k=5 q=71 b=1024 L=1e4: walk %.2f ms  tiles %.2f ms  (tiles / walk %.1fx)" % (tw, tt, tt / tw), flush=True)
    del E
    A, pi = model(1027, "band")
    t = {}
    for L in (6, 38):
        E = logE_of(1024, L, 1027)
        t[L] = timed(0, A, pi, E)
        del E
    print("config 5 q=1027 b=1024: L=6 %.3f ms, L=38 %.3f ms -> %.1f us per position" % (
        t[6], t[38], 1e3 * (t[38] - t[6]) / 32), flush=True)


if __name__ == "__main__":
    main()
