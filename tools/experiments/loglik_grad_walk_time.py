"""What the training walk with the sparse step for 65..256 states (hmm_loglik_grad_walk) costs next to what training
runs in this range today, and where hmm_loglik_grad_walk_pays may say 1.

Per step (a model, a batch), in ONE process, after a warm-up of every variant, timed with device events, the variants
ALTERNATING round by round so that drift hits them alike; every variant goes through the C ABI on buffers allocated
once (the two gradient calls share one dE):
  (a)  hmm_loglik_grad_large at its default route   the dense walk up to 128 states, per-position GEMMs above
  (b)  hmm_loglik_grad_walk, gradients              forward sweep + backward sweep + the sums
  (c)  engine.forward(want_log_alpha=False)         what autograd.LogLikelihood.forward runs: per-position GEMMs
  (d)  hmm_loglik_grad_walk, log-likelihood alone   the forward sweep without the store of dE
Reported per variant: the fastest round, the median, the spread (slowest - fastest); the sweeps separately: the
forward sweep is (d), the backward sweep with the sums is median (b) - median (d) (derived, not timed on its own).
The rule: a cell pays where median (a) / median (b) >= 1.25 (the margin of every _pays of the project); `--table`
folds the step lines of a run into the table of profiles/loglik_grad_walk.json.  (b) is compared with (a) on the same
inputs: the largest difference of dA on present edges, of dpi, dE and loglik, each over the tensor's largest entry,
and how many entries of (b)'s dA off the support are not exactly 0.

Steps: the 71-, 127- and 253-state gene models at b = 1, 32, 1024 x L = 10 000, emissions 0.05 + 0.9 u^4, weights
0.5 + u.  One child process per step under its own time limit; the first failure stops the run.  One JSON line per step.

    python tools/experiments/loglik_grad_walk_time.py [--steps g71-32,...] [--rounds N] [--L 10000] [--out FILE]
    python tools/experiments/loglik_grad_walk_time.py --table FILE        the pays table of the step lines in FILE
"""
import json
import os
import statistics
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from hmm_layer_amd import engine  # noqa: E402

DEV = "cuda:0"
STEPS = tuple("g%d-%d" % (q, b) for q in (71, 127, 253) for b in (1, 32, 1024))
MARGIN = 1.25


def model(q):
    from hmm_layer_amd.gene_pred_hmm_transitioner import GenePredMultiHMMTransitioner
    tr = GenePredMultiHMMTransitioner(k=(q - 1) // 14, initial_exon_len=200, initial_intron_len=4500,
                                      initial_ir_len=10000, starting_distribution_init="zeros").to(DEV)
    with torch.no_grad():
        A, pi = tr.make_A().contiguous(), tr.make_initial_distribution().reshape(1, -1).contiguous()
    assert A.shape[-1] == q
    return A.float(), pi.float()


def one(step, rounds, L):
    name, b = step.split("-")
    q, b = int(name[1:]), int(b)
    A, pi = model(q)
    g = torch.Generator(device=DEV).manual_seed(7)
    E = torch.rand((1, b, L, q), device=DEV, generator=g).pow_(4).mul_(0.9).add_(0.05)
    w = torch.rand((1, b), device=DEV, generator=g) + 0.5
    lib = engine.lib()
    dims = (1, b, L, q)
    dE = torch.empty_like(E)
    outs = {n: (torch.empty((1, q, q), device=DEV), torch.empty((1, q), device=DEV),
                torch.empty((1, b), dtype=torch.float64, device=DEV)) for n in ("large", "walk")}
    ll_only = torch.empty((1, b), dtype=torch.float64, device=DEV)
    ws_large = torch.empty(lib.hmm_loglik_grad_large_workspace_bytes(*dims), dtype=torch.uint8, device=DEV)
    ws_walk = torch.empty(lib.hmm_loglik_grad_walk_workspace_bytes(*dims), dtype=torch.uint8, device=DEV)

    def call(fn, ws, dA, dpi, dEt, ll, wt):
        rc = fn(A.data_ptr(), pi.data_ptr(), E.data_ptr(), *dims, engine.EPS, wt, dA, dpi, dEt, ll, ws.data_ptr(),
                ws.numel(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc

    def va():
        dA, dpi, ll = outs["large"]
        call(lib.hmm_loglik_grad_large, ws_large, dA.data_ptr(), dpi.data_ptr(), dE.data_ptr(), ll.data_ptr(), w.data_ptr())

    def vb():
        dA, dpi, ll = outs["walk"]
        call(lib.hmm_loglik_grad_walk, ws_walk, dA.data_ptr(), dpi.data_ptr(), dE.data_ptr(), ll.data_ptr(), w.data_ptr())

    def vc():
        return engine.forward(A, pi, E, want_log_alpha=False)

    def vd():
        call(lib.hmm_loglik_grad_walk, ws_walk, None, None, None, ll_only.data_ptr(), None)

    variants = (("loglik_grad_large", va), ("loglik_grad_walk", vb), ("forward_gemm", vc), ("loglik_walk", vd))
    for _, fn in variants:                                   # warm-up: workspaces, code objects, the allocator
        fn()
        fn()
    torch.cuda.synchronize()
    refused = lib.hmm_loglik_grad_walk_refused(*dims, ws_walk.data_ptr(), ws_walk.numel())
    assert refused == 0, refused
    times = {n: [] for n, _ in variants}
    for _ in range(rounds):
        for n, fn in variants:
            a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            z.record()
            z.synchronize()
            times[n].append(a.elapsed_time(z))
    rec = {"step": step, "q": q, "b": b, "L": L, "rounds": rounds,
           "large_route": "walk" if q <= 128 else "gemm"}
    for n, _ in variants:
        t = times[n]
        rec[n + "_ms"] = {"min": round(min(t), 4), "median": round(statistics.median(t), 4),
                          "spread": round(max(t) - min(t), 4)}
    med = lambda n: rec[n + "_ms"]["median"]                  # noqa: E731
    rec["forward_sweep_ms"] = med("loglik_walk")
    rec["backward_sweep_and_sums_ms"] = round(med("loglik_grad_walk") - med("loglik_walk"), 4)
    rec["grad_large_over_walk"] = round(med("loglik_grad_large") / med("loglik_grad_walk"), 3)
    rec["forward_gemm_over_loglik_walk"] = round(med("forward_gemm") / med("loglik_walk"), 3)
    rec["pays"] = int(rec["grad_large_over_walk"] >= MARGIN)
    # (b) against (a) on the same inputs
    va()
    big = [t.clone() for t in outs["large"]] + [dE[0, :min(b, 4)].clone()]
    vb()
    torch.cuda.synchronize()
    got = list(outs["walk"]) + [dE[0, :min(b, 4)]]
    on = A != 0
    rec["dA_present_max_rel_diff"] = float(((got[0] - big[0]).abs() * on).max() / big[0].abs().max())
    rec["dA_off_support_nonzero"] = int((got[0][~on] != 0).sum())
    rec["dpi_max_rel_diff"] = float((got[1] - big[1]).abs().max() / big[1].abs().max())
    rec["dE_max_rel_diff"] = float((got[3] - big[3]).abs().max() / big[3].abs().max())
    rec["loglik_max_rel_diff"] = float(((got[2] - big[2]).abs() / big[2].abs()).max())
    rec["loglik_forms_equal"] = bool(torch.equal(ll_only, got[2]))
    print(json.dumps(rec), flush=True)


def pays_table(path):
    """The step lines of a run -> {q: {b: ratios and pays}}."""
    recs = [json.loads(x) for x in open(path) if x.startswith("{")]
    out = {}
    for r in recs:
        out.setdefault(str(r["q"]), {})[str(r["b"])] = {
            "grad_large_over_walk": r["grad_large_over_walk"],
            "forward_gemm_over_loglik_walk": r["forward_gemm_over_loglik_walk"], "pays": r["pays"]}
    return out


def main():
    arg = lambda flag: sys.argv[sys.argv.index(flag) + 1] if flag in sys.argv else None   # noqa: E731
    if arg("--table"):
        print(json.dumps(pays_table(arg("--table")), indent=1))
        return
    rounds, L = int(arg("--rounds") or 7), int(arg("--L") or 10000)
    if arg("--one"):
        return one(arg("--one"), rounds, L)
    limit = int(arg("--limit") or 240)
    for step in (arg("--steps") or ",".join(STEPS)).split(","):
        # a child process per step, each under its own time limit; the first failure stops the run
        res = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", step, "--rounds", str(rounds),
                              "--L", str(L)], capture_output=True, text=True, timeout=limit)
        if res.returncode != 0:
            print(res.stdout + res.stderr[-2000:], flush=True)
            sys.exit("step %s ended with status %d: stopping" % (step, res.returncode))
        line = [x for x in res.stdout.splitlines() if x.startswith("{")][-1]
        print(line, flush=True)
        if arg("--out"):
            with open(arg("--out"), "a") as fh:
                fh.write(line + "\n")


if __name__ == "__main__":
    main()
