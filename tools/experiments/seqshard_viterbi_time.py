"""Sequence-sharded Viterbi on ONE GPU: what the three local calls cost, ranks played in turn, collectives not included.

For b = 1 x L = 1e6 and b = 4 x L = 250 000 at 15 states (the gene model):
  (a) engine.viterbi on the whole tensor — with --parent-lib PATH also through a library built from the parent commit
      (a child process: one library per process), to show the unsharded call has not moved;
  (b) the three calls with R = 1;
  (c) R = 8 equal slabs, each rank's own time for its reduce + apply + path (a stream and a workspace per rank).
Paths and scores of (b) and (c) must equal (a)'s.  Prints one JSON line per shape; the projected ratio is
(a) / max over ranks of (c): two real ranks, and the three all-gathers, are NOT measured here.

    python tools/experiments/seqshard_viterbi_time.py [--parent-lib /path/to/libhmm_engine.so]
"""
import json
import os
import subprocess
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from hmm_layer_amd import engine  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _model import gene15  # noqa: E402

DEV = "cuda:0"
SHAPES = ((1, 1000000), (4, 250000))
Q, R8, REPS = 15, 8, 5


def timed(fn, reps=REPS):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3, out


def inputs(b, L):
    A, pi = gene15(DEV)
    g = torch.Generator(device=DEV).manual_seed(5)
    logE = torch.log(torch.rand((1, b, L, Q), device=DEV, generator=g) * 0.9 + 0.05)
    return torch.log(A).reshape(1, Q, Q).contiguous(), torch.log(pi).reshape(1, Q).contiguous(), logE


def unsharded_only(lib_path):
    """Child process: (a) through another build of the library (it need not export the sharded entry points)."""
    engine.LIB_PATH = lib_path
    for name in [n for n in engine._SIGNATURES if n.startswith("hmm_seqshard_viterbi")]:
        del engine._SIGNATURES[name]
    for b, L in SHAPES:
        logA, logpi, logE = inputs(b, L)
        ms, _ = timed(lambda: engine.viterbi(logA, logpi, logE))
        print(json.dumps({"b": b, "L": L, "unsharded_ms": ms}), flush=True)


_streams = {}


def rank_stream(r):
    """One stream, hence one cached workspace, per rank for the whole run: no pass pays for its allocation again."""
    if r not in _streams:
        _streams[r] = torch.cuda.Stream()
    return _streams[r]


def sharded(logA, logpi, logE, R):
    """-> path (1,b,L), score, per-rank ms of (reduce, apply, path): every call timed on its own, ranks in turn."""
    L = logE.shape[2]
    cuts = [L * r // R for r in range(R + 1)]
    slabs = [logE[:, :, cuts[r]:cuts[r + 1]].contiguous() for r in range(R)]
    streams = [rank_stream(r) for r in range(R)]
    ms = [[0.0, 0.0, 0.0] for _ in range(R)]

    def on(r, i, fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.cuda.stream(streams[r]):
            out = fn()
        torch.cuda.synchronize()
        ms[r][i] = (time.perf_counter() - t0) * 1e3
        return out

    red = [on(r, 0, lambda: engine.seqshard_viterbi_reduce(logA, logpi, slabs[r], r == 0, R)) for r in range(R)]
    all_vops = torch.stack([v for v, _ in red], dim=2).contiguous()
    all_vbases = torch.stack([v for _, v in red], dim=2).contiguous()
    app = [on(r, 1, lambda: engine.seqshard_viterbi_apply(logA, logpi, slabs[r], all_vops, all_vbases, r))
           for r in range(R)]
    all_origins = torch.stack([o for o, _, _ in app], dim=2).contiguous()
    paths = [on(r, 2, lambda: engine.seqshard_viterbi_path(tuple(slabs[r].shape), all_origins, app[r][1], r))
             for r in range(R)]
    return torch.cat(paths, dim=2), app[0][2], ms


def main():
    if "--lib" in sys.argv:
        return unsharded_only(sys.argv[sys.argv.index("--lib") + 1])
    parent = {}
    if "--parent-lib" in sys.argv:
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--lib", sys.argv[sys.argv.index("--parent-lib") + 1]],
                             check=True, capture_output=True, text=True).stdout
        for line in out.splitlines():
            rec = json.loads(line)
            parent[(rec["b"], rec["L"])] = rec["unsharded_ms"]
    for b, L in SHAPES:
        logA, logpi, logE = inputs(b, L)
        a_ms, (path, score) = timed(lambda: engine.viterbi(logA, logpi, logE))
        rec = {"b": b, "L": L, "states": Q, "a_unsharded_ms": a_ms, "a_parent_unsharded_ms": parent.get((b, L))}
        for R in (1, R8):
            best = None
            for _ in range(3):                               # first pass warms the workspaces up; keep the fastest
                p, s, ms = sharded(logA, logpi, logE, R)
                assert torch.equal(p, path) and torch.equal(s, score), "sharded result differs"
                tot = [sum(m) for m in ms]
                if best is None or max(tot) < max(sum(m) for m in best):
                    best = ms
            rec["R%d_rank_ms" % R] = [round(sum(m), 4) for m in best]
            rec["R%d_reduce_apply_path_ms" % R] = [[round(x, 4) for x in m] for m in best]
        rec["projected_ratio_a_over_max_rank_R8"] = a_ms / max(rec["R%d_rank_ms" % R8])
        rec["note"] = "one GPU, ranks in turn, collectives not included; two real ranks unmeasured"
        print(json.dumps(rec), flush=True)
        del logE, path, score
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
