"""hmm_posterior_grad (17..64 states: four whole-sequence sweeps, one workgroup per sequence) against
hmm_posterior_grad_scan (per chunk of the scan plan) in one process: the table behind hmm_posterior_grad_scan_pays
(DESIGN 12c).  The protocol is tools/experiments/llgrad_scan_time.py's.

    python tools/experiments/postgrad_scan_time.py [--out FILE] [--calls 20] [--models dense24,gene43,gene57,dense64]
                                                   [--shapes 32x9999,...]

Without --model the script is a driver: every (model, shape) runs in a child process of its own under `timeout`, one
after the other, and the first child that fails ends the run.  A child times one call of each entry point first and
gives up by itself (status 3, no kill; the driver goes on to the next shape) if the remaining calls would not fit well
inside its limit; otherwise it alternates the two entry points call by call (device events around each call, warm-up
first) and prints the medians, the ratio, how many sequences the scan handed back to the sweeps and the largest
relative difference between the two results.  Mode: log; the upstream gradient is the cross-entropy against the most
probable state (-1 there, 0 elsewhere).  hmm_posterior_grad is called through the C ABI directly, so the figures do not
depend on what engine.posterior_grad routes where."""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

MODELS = ("dense24", "gene43", "gene57", "dense64")
SHAPES = ((1, 100000), (4, 100000), (16, 100000), (32, 9999), (64, 9999), (128, 9999), (512, 9999),
          (8, 2000))                                  # the last one: how far down in L the rule may reach
CHILD_SECONDS = 120                                   # per (model, shape): start-up, inputs, 2 * (3 + calls) calls
CALLS_SECONDS = 60                                    # what the child lets its own calls take of that


def model(name, dev):
    import torch
    q = int(name[-2:])
    g = torch.Generator().manual_seed(q)
    if name.startswith("gene"):
        from hmm_layer_amd.gene_pred_hmm_transitioner import GenePredMultiHMMTransitioner
        tr = GenePredMultiHMMTransitioner(k={43: 3, 57: 4}[q], initial_exon_len=200, initial_intron_len=4500,
                                          initial_ir_len=10000)
        with torch.no_grad():
            A = tr.make_A()[0].float()
    else:
        A = torch.rand((q, q), generator=g) ** 2 + 1e-2
        A = A / A.sum(-1, keepdim=True)
    assert A.shape == (q, q)
    return A[None].contiguous().to(dev), torch.full((1, q), 1.0 / q, device=dev), q


def child(name, shapes, calls, out):
    import time
    import torch
    from hmm_layer_amd import engine
    dev = torch.device("cuda:0")
    lib = engine.lib()
    A, pi, q = model(name, dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    for b, L in shapes:
        dims = (1, b, L, q)
        g = torch.Generator(device=dev).manual_seed(b * 7 + L)
        E = torch.rand((1, b, L, q), device=dev, generator=g) * 0.9 + 0.05
        gamma = engine.posterior(A, pi, E, mode=engine.POST_PROB)[0]
        G = -torch.nn.functional.one_hot(gamma.argmax(-1), q).to(torch.float32).contiguous()
        del gamma
        res = {}
        for fn in ("hmm_posterior_grad", "hmm_posterior_grad_scan"):
            need = getattr(lib, fn + "_workspace_bytes")(*dims)
            assert need > 0, (fn, dims)
            res[fn] = dict(ws=torch.empty(need, dtype=torch.uint8, device=dev), dA=torch.empty((1, q, q), device=dev),
                           dpi=torch.empty((1, q), device=dev), dE=torch.empty_like(E), ms=[])

        def run(fn):
            r = res[fn]
            rc = getattr(lib, fn)(A.data_ptr(), pi.data_ptr(), E.data_ptr(), *dims, engine.EPS, engine.POST_LOG,
                                  G.data_ptr(), r["dA"].data_ptr(), r["dpi"].data_ptr(), r["dE"].data_ptr(),
                                  r["ws"].data_ptr(), r["ws"].numel(), stream)
            assert rc == 0, (fn, rc)

        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for fn in res:
            run(fn)
        torch.cuda.synchronize()
        first = time.perf_counter() - t0                      # one call of each, with what a first call adds
        if first * (2 + calls) > CALLS_SECONDS:
            print("postgrad_scan_time: %s b=%d L=%d: a call of each takes %.2f s, %d more do not fit %d s"
                  % (name, b, L, first, 2 + calls, CALLS_SECONDS), flush=True)
            return 3
        for _ in range(2):
            for fn in res:
                run(fn)
        torch.cuda.synchronize()
        for _ in range(calls):
            for fn in res:                                    # alternating: both see the same machine
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run(fn)
                e1.record()
                e1.synchronize()
                res[fn]["ms"].append(e0.elapsed_time(e1))
        redone = int(lib.hmm_posterior_grad_scan_serial_count(*dims, res["hmm_posterior_grad_scan"]["ws"].data_ptr(),
                                                              res["hmm_posterior_grad_scan"]["ws"].numel()))
        a, s = res["hmm_posterior_grad"], res["hmm_posterior_grad_scan"]
        diff = max(float((a[t] - s[t]).abs().max() / a[t].abs().max()) for t in ("dA", "dpi", "dE"))
        ma, ms = statistics.median(a["ms"]), statistics.median(s["ms"])
        rec = dict(model=name, q=q, b=b, L=L, chunk=lib.hmm_posterior_grad_scan_chunk_len(*dims), calls=calls,
                   posterior_grad_ms=round(ma, 4), posterior_grad_min_max=[round(min(a["ms"]), 4), round(max(a["ms"]), 4)],
                   scan_ms=round(ms, 4), scan_min_max=[round(min(s["ms"]), 4), round(max(s["ms"]), 4)],
                   speedup=round(ma / ms, 3), redone=redone, max_rel_diff=diff,
                   grad_takes_chunks=bool(lib.hmm_posterior_grad_serial_count(*dims, a["ws"].data_ptr(), a["ws"].numel()) < b),
                   pays=int(lib.hmm_posterior_grad_scan_pays(*dims)))
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            with open(out, "a") as fh:
                fh.write(line + "\n")
        del res, E, G
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model")
    ap.add_argument("--models", default=",".join(MODELS))
    ap.add_argument("--shapes", default=",".join("%dx%d" % s for s in SHAPES))
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.calls < 20:
        ap.error("at least 20 timed calls per entry point")
    shapes = [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")]
    if a.model:
        return child(a.model, shapes, a.calls, a.out)
    for name in a.models.split(","):
        for b, L in shapes:
            cmd = ["timeout", "-k", "10", str(CHILD_SECONDS), sys.executable, os.path.abspath(__file__), "--model", name,
                   "--shapes", "%dx%d" % (b, L), "--calls", str(a.calls)] + (["--out", a.out] if a.out else [])
            rc = subprocess.run(cmd).returncode
            if rc == 3:                                       # the child declined by itself: no fault, the next shape
                continue
            if rc != 0:
                print("postgrad_scan_time: %s b=%d L=%d ended with status %d; nothing more is started" % (name, b, L, rc),
                      flush=True)
                return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
