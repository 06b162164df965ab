"""Chunk length against rounds of resident blocks, one process, two rounds:
   python rounds_sweep.py [--b 1024 --len 100000 --states 15] [--lo 256 --hi 512] [--ab]
Runs the posterior at every forced chunk length T (OPT_CHUNK) that is a multiple of 16 in [lo, hi], then at the
default plan (T = 0), and prints per-kernel HIP-event times (engine.Profile), the whole pass, the plan's chunks per
sequence and its rounds of resident blocks (apply kernels: 2 blocks of 4 waves per CU, sparse reduce: 4; 256 CUs).
With --ab only OPT_CHUNK = 512 and the default plan alternate (the "done when" comparison of the chunk rule).
profiles/rounds_sweep.txt is three processes of it."""
import argparse, os, sys, time, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from hmm_layer_amd import engine
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _model import gene15

ap = argparse.ArgumentParser()
ap.add_argument("--b", type=int, default=1024)
ap.add_argument("--len", type=int, default=100000)
ap.add_argument("--states", type=int, default=15)
ap.add_argument("--lo", type=int, default=256)
ap.add_argument("--hi", type=int, default=512)
ap.add_argument("--ab", action="store_true")
ap.add_argument("--reps", type=int, default=5)
args = ap.parse_args()
dev = torch.device('cuda:0')
b, L, q = args.b, args.len, args.states
if q == 15:
    A, pi = gene15(dev)
else:
    g = torch.Generator(device=dev).manual_seed(1)
    A = torch.rand((1, q, q), device=dev, generator=g) + 0.05
    A = (A / A.sum(-1, keepdim=True)).contiguous()
    pi = torch.full((1, q), 1.0 / q, device=dev)
E = torch.rand((1, b, L, q), device=dev) * 0.9 + 0.05
out = torch.empty_like(E)
Ts = [512, 0] if args.ab else list(range(args.lo, args.hi + 1, 16)) + [0]
for rnd in range(2):
    for T in Ts:
        engine.release_workspaces()
        engine.set_option(engine.OPT_CHUNK, T)
        t_eff = engine.chunk_len(1, b, L, q)
        C = (L + t_eff - 1) // t_eff
        blocks = (b * C + 63) // 64
        prof = engine.Profile()
        engine.posterior(A, pi, E, out=out)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for r in range(args.reps):
            engine.posterior(A, pi, E, out=out, profile=prof)
        torch.cuda.synchronize(); dt = (time.perf_counter() - t0) / args.reps
        ms = {n: round(v[0] / max(v[1], 1), 3) for n, v in prof.read().items()}
        t1 = time.perf_counter()
        for r in range(args.reps): engine.forward(A, pi, E, want_log_alpha=False)
        torch.cuda.synchronize(); dl = (time.perf_counter() - t1) / args.reps
        print("round %d T=%-7s C=%4d rounds apply %6.3f reduce %6.3f" % (rnd, ("%d" % T) if T else "def:%d" % t_eff, C, blocks / 512,
              (b * C + 15) // 16 / 1024), ms, "pass %.3f ms  loglik %.3f ms" % (dt * 1e3, dl * 1e3),
              "chk %.6f" % float(out[0, ::97, ::997].double().sum()), flush=True)
        prof.close()
engine.set_option(engine.OPT_CHUNK, 0)
