"""hmm_viterbi_scan (engine.viterbi_scan) against hmm_viterbi's one-wave-per-sequence walk, 17..64 states.

  python tools/experiments/vit_scan_time.py [--quick | --prof] [--out FILE]

The walk is timed through lib().hmm_viterbi directly, which never takes the scan.  Models: the 29-, 43- and
57-state gene models (two to four copies) and a dense 48-state model.  Shapes: b = 1, 4, 16, 64, 256, 1024 x
L = 1e5 and b = 1 x L = 1e6.  Per shape and path: one warm-up call, then five timed calls (host clock around a call
that ends in a device synchronise); printed are the median, the minimum and the maximum in milliseconds, and
whether the scan won by more than the spread (scan max < walk min): the rule hmm_viterbi_scan_pays is derived from.
Both results are compared bit for bit at every shape.
--quick: b = 1, 16 x L = 1e5 and b = 1 x L = 1e6 on the 29- and 43-state models.
--prof: one call each of scan and walk on the 29-state model at b = 1 x L = 1e6 and b = 1 x L = 1e5 (for
rocprofv3 --kernel-trace --stats, in a run of its own)."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from hmm_layer_amd import engine  # noqa: E402
from tests import viterbi_wide as vw  # noqa: E402

dev = torch.device("cuda:0")


def gene(copies):
    from hmm_layer_amd.gene_pred_hmm_transitioner import GenePredMultiHMMTransitioner
    tr = GenePredMultiHMMTransitioner(k=copies, initial_exon_len=200, initial_intron_len=4500, initial_ir_len=10000)
    with torch.no_grad():
        return (torch.log(tr.make_A()).to(dev).contiguous(),
                torch.log(tr.make_initial_distribution().reshape(1, -1)).to(dev).contiguous())


def dense(q):
    logA, logpi = vw.random_model(np.random.default_rng(q), q, "dense")
    return torch.tensor(logA, device=dev)[None].contiguous(), torch.tensor(logpi, device=dev)[None].contiguous()


def logE_of(b, L, q):
    g = torch.Generator(device=dev).manual_seed(b + L + q)
    return torch.rand((1, b, L, q), generator=g, device=dev).mul_(-6)


def walk(A, pi, E, ws):
    lib = engine.lib()
    k, b, L, q = E.shape
    path = torch.empty((k, b, L), dtype=torch.int32, device=dev)
    score = torch.empty((k, b), dtype=torch.float64, device=dev)
    rc = lib.hmm_viterbi(A.data_ptr(), pi.data_ptr(), E.data_ptr(), k, b, L, q, path.data_ptr(), score.data_ptr(),
                         ws.data_ptr(), ws.numel(), engine._stream(dev))
    assert rc == 0, rc
    return path, score


def timed(fn, reps=5):
    out = fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    return out, ts


def main():
    quick, prof = "--quick" in sys.argv, "--prof" in sys.argv
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    models = [("gene29", gene(2)), ("gene43", gene(3))]
    shapes = [(1, 100000), (16, 100000), (1, 1000000)]
    if not quick and not prof:
        models += [("gene57", gene(4)), ("dense48", dense(48))]
        shapes = [(b, 100000) for b in (1, 4, 16, 64, 256, 1024)] + [(1, 1000000)]
    if prof:
        models, shapes = models[:1], [(1, 1000000), (1, 100000)]
    rows = []
    for name, (A, pi) in models:
        q = A.shape[-1]
        for b, L in shapes:
            E = logE_of(b, L, q)
            ws = torch.empty(max(engine.lib().hmm_viterbi_workspace_bytes(1, b, L, q), 256), dtype=torch.uint8, device=dev)
            (ps, ss), ts = timed(lambda: engine.viterbi_scan(A, pi, E), 1 if prof else 5)
            (pw, sw), tw = timed(lambda: walk(A, pi, E, ws), 1 if prof else 5)
            same = bool(torch.equal(ps, pw) and torch.equal(ss, sw))
            row = dict(model=name, q=q, b=b, L=L, chunk=engine.lib().hmm_viterbi_scan_chunk_len(1, b, L, q),
                       scan_ms=[round(t, 4) for t in ts], walk_ms=[round(t, 4) for t in tw], identical=same,
                       scan_wins=bool(max(ts) < min(tw)), pays=int(engine.lib().hmm_viterbi_scan_pays(1, b, L, q)))
            rows.append(row)
            print("%-8s q=%2d b=%4d L=%7d T=%3d: scan %9.3f [%9.3f, %9.3f] ms   walk %9.3f [%9.3f, %9.3f] ms   "
                  "%s  identical=%s pays=%d" % (name, q, b, L, row["chunk"], np.median(ts), min(ts), max(ts),
                                               np.median(tw), min(tw), max(tw),
                                               "SCAN" if row["scan_wins"] else "walk", same, row["pays"]), flush=True)
            del E, ws, ps, ss, pw, sw
            engine.release_workspaces()
            torch.cuda.empty_cache()
    if out:
        with open(out, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
