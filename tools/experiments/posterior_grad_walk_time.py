"""What the posterior-gradient walk with the sparse step for 65..256 states (hmm_posterior_grad_walk) costs next to
what training through the posteriors runs in this range today, and where hmm_posterior_grad_walk_pays may say 1.

Per step (a model, a batch), in ONE process, after a warm-up of every variant, timed with device events, the variants
ALTERNATING round by round so that drift hits them alike.  Log mode, a label-style upstream gradient
(-(rand < 0.05) / (b L), the gradient of a mean cross-entropy against labels):
  (a)  hmm_posterior_grad_large at its default route   the dense walk up to 128 states, per-position GEMMs above
  (b)  hmm_posterior_grad_walk                         four sweeps + the sums
  (c)  autograd.posterior, forward + backward          today's node: hmm_posterior's GEMMs, then (a)
  (d)  autograd.posterior(support_only="always")       the new node: hmm_posterior_walk, then (b)
(a) and (b) go through the C ABI on buffers allocated once (they share one dE); (c) and (d) run as training runs
them, allocations included.  Reported per variant: the fastest round, the median, the spread (slowest - fastest).
The rule: a cell pays where median (a) / median (b) >= 1.25 (the margin of every _pays of the project); `--table`
folds the step lines of a run into the table of profiles/posterior_grad_walk.json.  (b) is compared with (a) on the
same inputs: the largest difference of dA on present edges, of dpi and dE, each over the tensor's largest entry, and
how many entries of (b)'s dA off the support are not exactly 0.

Steps: the 71-, 127- and 253-state gene models at b = 1, 32, 1024 x L = 10 000, emissions 0.05 + 0.9 u^4.  One child
process per step under its own time limit; the first failure stops the run.  One JSON line per step.

    python tools/experiments/posterior_grad_walk_time.py [--steps g71-32,...] [--rounds N] [--L 10000] [--out FILE]
    python tools/experiments/posterior_grad_walk_time.py --table FILE        the pays table of the step lines in FILE
"""
import json
import os
import statistics
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from hmm_layer_amd import autograd, engine  # noqa: E402

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
    G = -(torch.rand((1, b, L, q), device=DEV, generator=g) < 0.05).float() / (b * L)
    lib = engine.lib()
    dims = (1, b, L, q)
    dE = torch.empty_like(E)
    outs = {n: (torch.empty((1, q, q), device=DEV), torch.empty((1, q), device=DEV)) for n in ("large", "walk")}
    ws_large = torch.empty(lib.hmm_posterior_grad_large_workspace_bytes(*dims), dtype=torch.uint8, device=DEV)
    ws_walk = torch.empty(lib.hmm_posterior_grad_walk_workspace_bytes(*dims), dtype=torch.uint8, device=DEV)

    def call(fn, ws, dA, dpi):
        rc = fn(A.data_ptr(), pi.data_ptr(), E.data_ptr(), *dims, engine.EPS, engine.POST_LOG, G.data_ptr(),
                dA.data_ptr(), dpi.data_ptr(), dE.data_ptr(), ws.data_ptr(), ws.numel(),
                torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc

    def va():
        call(lib.hmm_posterior_grad_large, ws_large, *outs["large"])

    def vb():
        call(lib.hmm_posterior_grad_walk, ws_walk, *outs["walk"])

    def node(support):
        leaves = [t.detach().requires_grad_(True) for t in (A, pi, E)]
        out = autograd.posterior(*leaves, mode=engine.POST_LOG, support_only=support)
        out.backward(G)

    variants = (("posterior_grad_large", va), ("posterior_grad_walk", vb), ("autograd_default", lambda: node(False)),
                ("autograd_support", lambda: node("always")))
    for _, fn in variants:                                   # warm-up: workspaces, code objects, the allocator
        fn()
        fn()
    torch.cuda.synchronize()
    refused = lib.hmm_posterior_grad_walk_refused(*dims, ws_walk.data_ptr(), ws_walk.numel())
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
    rec = {"step": step, "q": q, "b": b, "L": L, "rounds": rounds, "mode": "log", "G": "label",
           "large_route": "walk" if q <= 128 else "gemm"}
    for n, _ in variants:
        t = times[n]
        rec[n + "_ms"] = {"min": round(min(t), 4), "median": round(statistics.median(t), 4),
                          "spread": round(max(t) - min(t), 4)}
    med = lambda n: rec[n + "_ms"]["median"]                  # noqa: E731
    rec["grad_large_over_walk"] = round(med("posterior_grad_large") / med("posterior_grad_walk"), 3)
    rec["autograd_default_over_support"] = round(med("autograd_default") / med("autograd_support"), 3)
    rec["pays"] = int(rec["grad_large_over_walk"] >= MARGIN)
    # (b) against (a) on the same inputs
    va()
    big = [t.clone() for t in outs["large"]] + [dE[0, :min(b, 4)].clone()]
    vb()
    torch.cuda.synchronize()
    got = list(outs["walk"]) + [dE[0, :min(b, 4)]]
    on = A != 0
    rec["dA_present_max_rel_diff"] = float(((got[0] - big[0]).abs() * on).max() / (big[0].abs() * on).max())
    rec["dA_off_support_nonzero"] = int((got[0][~on] != 0).sum())
    rec["dpi_max_rel_diff"] = float((got[1] - big[1]).abs().max() / big[1].abs().max())
    rec["dE_max_rel_diff"] = float((got[2] - big[2]).abs().max() / big[2].abs().max())
    print(json.dumps(rec), flush=True)


def pays_table(path):
    """The step lines of a run -> {q: {b: ratios and pays}}."""
    recs = [json.loads(x) for x in open(path) if x.startswith("{")]
    out = {}
    for r in recs:
        out.setdefault(str(r["q"]), {})[str(r["b"])] = {
            "grad_large_over_walk": r["grad_large_over_walk"],
            "autograd_default_over_support": r["autograd_default_over_support"], "pays": r["pays"]}
    return out


def main():
    arg = lambda flag: sys.argv[sys.argv.index(flag) + 1] if flag in sys.argv else None   # noqa: E731
    if arg("--table"):
        print(json.dumps(pays_table(arg("--table")), indent=1))
        return
    rounds, L = int(arg("--rounds") or 7), int(arg("--L") or 10000)
    if arg("--one"):
        return one(arg("--one"), rounds, L)
    limit = int(arg("--limit") or 300)
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
