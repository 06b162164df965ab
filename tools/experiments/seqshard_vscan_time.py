"""Sequence-sharded Viterbi for 17-64 states on ONE GPU: what the three local calls cost, ranks played in turn,
collectives not included.

For the 29- and 43-state gene models and a dense 48-state model, at b = 1 x L = 1e6 and b = 4 x L = 250 000:
  (a) hmm_viterbi (the one-wave-per-sequence walk) and engine.viterbi_scan on the whole tensor;
  (b) the three calls with R = 1;
  (c) R = 8 equal slabs, each rank's own time for its reduce + apply + path (a stream and a workspace per rank).
Every figure is the fastest of three passes after a warm-up, with a device synchronisation around each call.  Paths
and scores of (b) and (c) must equal (a)'s.  Prints one JSON line per (model, shape); the projected ratios are
(a) / max over ranks of (c): two real ranks, and the three all-gathers, are NOT measured here.

    python tools/experiments/seqshard_vscan_time.py [--models g29,g43,d48] [--out FILE]

Has the unsharded path moved?  engine.viterbi_scan at b = 1 x L = 1e6 (29 states) and b = 16 x L = 1e5 (43 states)
through two builds of the library, alternating, five timings each (one child process per timing: one library per
process; the parent build need not export the sharded entry points):

    python tools/experiments/seqshard_vscan_time.py --compare PARENT.so [--out FILE]
"""
import json
import os
import subprocess
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from hmm_layer_amd import engine  # noqa: E402

DEV = "cuda:0"
SHAPES = ((1, 1000000), (4, 250000))
COMPARE = (("g29", 1, 1000000), ("g43", 16, 100000))
R8, PASSES = 8, 3


def model(name):
    """-> logA (1,q,q), logpi (1,q) on the device: gQ the gene model of (Q - 1) / 14 copies, dQ a dense model."""
    q = int(name[1:])
    if name[0] == "g":
        from hmm_layer_amd.gene_pred_hmm_transitioner import GenePredMultiHMMTransitioner
        tr = GenePredMultiHMMTransitioner(k=(q - 1) // 14, initial_exon_len=200, initial_intron_len=4500,
                                          initial_ir_len=10000)
        with torch.no_grad():
            A, pi = tr.make_A()[0].to(DEV), tr.make_initial_distribution().reshape(-1).to(DEV)
    else:
        g = torch.Generator(device=DEV).manual_seed(q)
        A = torch.rand((q, q), device=DEV, generator=g) ** 3 + 1e-3
        A, pi = A / A.sum(-1, keepdim=True), torch.full((q,), 1.0 / q, device=DEV)
    assert A.shape == (q, q)
    return torch.log(A).reshape(1, q, q).contiguous(), torch.log(pi).reshape(1, q).contiguous()


def emissions(b, L, q):
    g = torch.Generator(device=DEV).manual_seed(5)
    return torch.log(torch.rand((1, b, L, q), device=DEV, generator=g) * 0.9 + 0.05)


def walk(logA, logpi, logE):
    """lib().hmm_viterbi directly: the walk, whatever engine.viterbi would route to."""
    lib = engine.lib()
    k, b, L, q = logE.shape
    ws = engine._workspace(logE.device, lib.hmm_viterbi_workspace_bytes(k, b, L, q), "walk")
    path = torch.empty((k, b, L), dtype=torch.int32, device=DEV)
    score = torch.empty((k, b), dtype=torch.float64, device=DEV)
    engine._check(lib.hmm_viterbi(logA.data_ptr(), logpi.data_ptr(), logE.data_ptr(), k, b, L, q, path.data_ptr(),
                                  score.data_ptr(), ws.data_ptr(), ws.numel(), engine._stream(logE.device)))
    return path, score


def timed(fn):
    """-> (ms of one synchronised call, its result)."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def fastest(fn, passes=PASSES):
    fn()                                                     # warm-up: workspaces, code objects
    best, out = None, None
    for _ in range(passes):
        ms, out = timed(fn)
        best = ms if best is None else min(best, ms)
    return best, out


_streams = {}


def rank_stream(r):
    """One stream, hence one cached workspace, per rank for the whole run: no pass pays for its allocation again."""
    if r not in _streams:
        _streams[r] = torch.cuda.Stream()
    return _streams[r]


def sharded(logA, logpi, logE, R):
    """-> path (1,b,L), score, per-rank ms of (reduce, apply, path): every call timed on its own, ranks in turn."""
    from hmm_layer_amd import seqshard_vscan as sv
    L = logE.shape[2]
    cuts = [L * r // R for r in range(R + 1)]
    slabs = [logE[:, :, cuts[r]:cuts[r + 1]].contiguous() for r in range(R)]
    ms = [[0.0, 0.0, 0.0] for _ in range(R)]

    def on(r, i, fn):
        def run():
            with torch.cuda.stream(rank_stream(r)):
                return fn()
        ms[r][i], out = timed(run)
        return out

    red = [on(r, 0, lambda: sv.reduce(logA, logpi, slabs[r], r == 0, R)) for r in range(R)]
    all_vops = torch.stack([v for v, _ in red], dim=2).contiguous()
    all_vbases = torch.stack([v for _, v in red], dim=2).contiguous()
    app = [on(r, 1, lambda: sv.apply(logA, logpi, slabs[r], all_vops, all_vbases, r)) for r in range(R)]
    all_origins = torch.stack([o for o, _, _ in app], dim=2).contiguous()
    paths = [on(r, 2, lambda: sv.path(tuple(slabs[r].shape), all_origins, app[r][1], r)) for r in range(R)]
    return torch.cat(paths, dim=2), app[0][2], ms


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as fh:
            fh.write(line + "\n")


def measure(names, out):
    for name in names:
        logA, logpi = model(name)
        q = logA.shape[-1]
        for b, L in SHAPES:
            logE = emissions(b, L, q)
            walk_ms, (path, score) = fastest(lambda: walk(logA, logpi, logE))
            scan_ms, (spath, sscore) = fastest(lambda: engine.viterbi_scan(logA, logpi, logE))
            assert torch.equal(spath, path) and torch.equal(sscore, score), "viterbi_scan differs from the walk"
            del spath
            rec = {"model": name, "b": b, "L": L, "a_walk_ms": round(walk_ms, 4), "a_viterbi_scan_ms": round(scan_ms, 4)}
            for R in (1, R8):
                best = None
                for i in range(PASSES + 1):                  # the first pass warms the workspaces up; keep the fastest
                    p, s, ms = sharded(logA, logpi, logE, R)
                    assert torch.equal(p, path) and torch.equal(s, score), "sharded result differs"
                    del p
                    if i and (best is None or max(sum(m) for m in ms) < max(sum(m) for m in best)):
                        best = ms
                rec["R%d_rank_ms" % R] = [round(sum(m), 4) for m in best]
                rec["R%d_reduce_apply_path_ms" % R] = [[round(x, 4) for x in m] for m in best]
            slow = max(rec["R%d_rank_ms" % R8])
            rec["projected_ratio_walk_over_max_rank_R8"] = round(walk_ms / slow, 3)
            rec["projected_ratio_scan_over_max_rank_R8"] = round(scan_ms / slow, 3)
            rec["note"] = "one GPU, ranks in turn, collectives not included; two real ranks unmeasured"
            emit(rec, out)
            del logE, path, score
            engine.release_workspaces()
            torch.cuda.empty_cache()


def scan_only(lib_path):
    """Child process: engine.viterbi_scan through the library at lib_path, the fastest of three calls per shape."""
    engine.LIB_PATH = lib_path
    for name, b, L in COMPARE:
        logA, logpi = model(name)
        logE = emissions(b, L, logA.shape[-1])
        ms, _ = fastest(lambda: engine.viterbi_scan(logA, logpi, logE))
        print(json.dumps({"model": name, "b": b, "L": L, "viterbi_scan_ms": round(ms, 4)}), flush=True)
        del logE
        engine.release_workspaces()
        torch.cuda.empty_cache()


def compare(parent_lib, out, repeats=5):
    res = {}
    for i in range(repeats):
        for tag, path in (("parent", parent_lib), ("this", engine.LIB_PATH)):
            text = subprocess.run([sys.executable, os.path.abspath(__file__), "--lib", path], check=True,
                                  capture_output=True, text=True, timeout=300).stdout
            for line in text.splitlines():
                rec = json.loads(line)
                res.setdefault((rec["model"], rec["b"], rec["L"]), {"parent": [], "this": []})[tag].append(rec["viterbi_scan_ms"])
    for (name, b, L), v in res.items():
        emit({"model": name, "b": b, "L": L, "parent_viterbi_scan_ms": v["parent"], "this_viterbi_scan_ms": v["this"]}, out)


def main():
    arg = lambda flag: sys.argv[sys.argv.index(flag) + 1] if flag in sys.argv else None
    if arg("--lib"):
        return scan_only(arg("--lib"))
    if arg("--compare"):
        return compare(arg("--compare"), arg("--out"))
    measure((arg("--models") or "g29,g43,d48").split(","), arg("--out"))


if __name__ == "__main__":
    main()
