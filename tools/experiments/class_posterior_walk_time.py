"""What training on CLASS posteriors costs for 65..256 states through the fused calls (hmm_class_posterior_walk,
hmm_class_posterior_grad_walk) next to the composition it replaces, in time and in memory, and where
hmm_class_posterior_walk_pays may say 1.

Per step (a model, a batch), in ONE process: first the peak of torch.cuda.max_memory_allocated of one forward +
backward of (a) and of (b), each after the workspaces and the allocator's cache were released; then, after a warm-up of
every variant, timing with device events, the variants ALTERNATING round by round so that drift hits them alike.  Log
mode, 6 classes (intergenic and five per copy), the upstream gradient of a mean cross-entropy against class labels:
Gc = -one_hot(label) / (b L).
  (a)  the composition        autograd.posterior(POST_PROB, support_only="always") + index_add_ over the state axis +
                              log + (Gc * .).sum(), forward + backward: what a user with class labels runs without the
                              fused calls, on the best existing path (hmm_posterior_walk, hmm_posterior_grad_walk);
                              written out here with torch ops, nothing of the fused calls' code is on it
  (b)  the fused node         autograd.class_posterior(mode=POST_LOG, support_only="always") + (Gc * .).sum()
  (c)  hmm_class_posterior_walk (out_prob and out_log) against hmm_posterior_walk(HMM_POST_PROB), the C calls alone
  (d)  hmm_class_posterior_grad_walk(HMM_POST_LOG) against hmm_posterior_grad_walk(HMM_POST_PROB) with the (k,b,L,q)
       upstream gradient of the same loss (Gc / P expanded to the states), the C calls alone on buffers allocated once
Reported per variant: the fastest round, the median, the spread (slowest - fastest).  The rule: a cell pays where
median (a) / median (b) >= 1.25 (the margin of every _pays of the project); `--table` folds the step lines of a run
into the table of profiles/class_posterior_walk.json.  (b) is compared with (a) on the same inputs: the largest
difference of dA on present edges, of dpi and dE, each over the tensor's largest entry.

Steps: the 71-, 127- and 253-state gene models at b = 1, 32, 1024 x L = 10 000, emissions 0.05 + 0.9 u^4.  One child
process per step under its own time limit; the first failure stops the run.  One JSON line per step.

    python tools/experiments/class_posterior_walk_time.py [--steps g71-32,...] [--rounds N] [--L 10000] [--out FILE]
    python tools/experiments/class_posterior_walk_time.py --table FILE        the pays table of the step lines in FILE
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
C = 6


def model(q):
    from hmm_layer_amd.gene_pred_hmm_transitioner import GenePredMultiHMMTransitioner
    tr = GenePredMultiHMMTransitioner(k=(q - 1) // 14, initial_exon_len=200, initial_intron_len=4500,
                                      initial_ir_len=10000, starting_distribution_init="zeros").to(DEV)
    with torch.no_grad():
        A, pi = tr.make_A().contiguous(), tr.make_initial_distribution().reshape(1, -1).contiguous()
    assert A.shape[-1] == q
    return A.float(), pi.float()


def gene_classes(q):
    """intergenic, then five classes per copy's 14 states (3, 3, 3, 3, 2 of them), shared by the copies."""
    return [0] + [1 + (i % 14) // 3 for i in range(q - 1)]


def one(step, rounds, L):
    import ctypes
    name, b = step.split("-")
    q, b = int(name[1:]), int(b)
    A, pi = model(q)
    table = gene_classes(q)
    idx = torch.tensor(table, dtype=torch.long, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(7)
    E = torch.rand((1, b, L, q), device=DEV, generator=g).pow_(4).mul_(0.9).add_(0.05)
    lab = torch.randint(0, C, (1, b, L), device=DEV, generator=g)
    Gc = torch.zeros((1, b, L, C), device=DEV).scatter_(-1, lab[..., None], -1.0 / (b * L))
    del lab
    lib = engine.lib()
    dims = (1, b, L, q)
    grads = {}

    def composed():
        leaves = [t.detach().requires_grad_(True) for t in (A, pi, E)]
        gamma = autograd.posterior(*leaves, mode=engine.POST_PROB, support_only="always")
        P = torch.zeros(gamma.shape[:-1] + (C,), dtype=gamma.dtype, device=gamma.device).index_add_(-1, idx, gamma)
        (Gc * torch.log(P)).sum().backward()
        grads["composed"] = [t.grad for t in leaves]

    def fused():
        leaves = [t.detach().requires_grad_(True) for t in (A, pi, E)]
        out = autograd.class_posterior(*leaves, table, C, mode=engine.POST_LOG, support_only="always")
        (Gc * out).sum().backward()
        grads["fused"] = [t.grad for t in leaves]

    # ---- memory first: one forward + backward each, from released workspaces and an empty cache
    rec = {"step": step, "q": q, "b": b, "L": L, "rounds": rounds, "mode": "log", "classes": C,
           "G": "label", "inputs_bytes": int(torch.cuda.memory_allocated())}
    for n, fn in (("composed", composed), ("fused", fused)):
        grads.clear()
        engine.release_workspaces()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        rec[n + "_peak_bytes"] = int(torch.cuda.max_memory_allocated())
    # (b) against (a) on the same inputs
    composed()
    torch.cuda.synchronize()
    on = A != 0
    big, got = grads["composed"], grads["fused"]
    rec["dA_present_max_rel_diff"] = float(((got[0] - big[0]).abs() * on).max() / (big[0].abs() * on).max())
    rec["dA_off_support_nonzero"] = int((got[0][~on] != 0).sum())
    rec["dpi_max_rel_diff"] = float((got[1] - big[1]).abs().max() / big[1].abs().max())
    rec["dE_max_rel_diff"] = float((got[2][0, :min(b, 4)] - big[2][0, :min(b, 4)]).abs().max()
                                   / big[2][0, :min(b, 4)].abs().max())
    del big, got
    grads.clear()
    engine.release_workspaces()
    torch.cuda.empty_cache()

    # ---- the C calls alone, on buffers allocated once
    st = lambda: torch.cuda.current_stream().cuda_stream     # noqa: E731
    ctab = (ctypes.c_int * q)(*table)
    out = torch.empty_like(E)                                # hmm_posterior_walk's gamma, then the shared dE
    P, Lg = torch.empty((1, b, L, C), device=DEV), torch.empty((1, b, L, C), device=DEV)
    ll = torch.empty((1, b), dtype=torch.float64, device=DEV)
    dA, dpi = torch.empty((1, q, q), device=DEV), torch.empty((1, q), device=DEV)
    ws = torch.empty(max(lib.hmm_posterior_walk_workspace_bytes(*dims), lib.hmm_class_posterior_walk_workspace_bytes(*dims),
                         lib.hmm_posterior_grad_walk_workspace_bytes(*dims),
                         lib.hmm_class_posterior_grad_walk_workspace_bytes(*dims, C)), dtype=torch.uint8, device=DEV)

    def walk():
        rc = lib.hmm_posterior_walk(A.data_ptr(), pi.data_ptr(), E.data_ptr(), *dims, engine.EPS, engine.POST_PROB,
                                    out.data_ptr(), ll.data_ptr(), ws.data_ptr(), ws.numel(), st())
        assert rc == 0, rc

    def class_walk():
        rc = lib.hmm_class_posterior_walk(A.data_ptr(), pi.data_ptr(), E.data_ptr(), *dims, engine.EPS, ctab, C,
                                          P.data_ptr(), Lg.data_ptr(), ll.data_ptr(), ws.data_ptr(), ws.numel(), st())
        assert rc == 0, rc

    class_walk()
    torch.cuda.synchronize()
    Gs = (Gc / P)[..., idx].contiguous()                     # the state-level upstream gradient of the same loss

    def grad_walk():
        rc = lib.hmm_posterior_grad_walk(A.data_ptr(), pi.data_ptr(), E.data_ptr(), *dims, engine.EPS, engine.POST_PROB,
                                         Gs.data_ptr(), dA.data_ptr(), dpi.data_ptr(), out.data_ptr(), ws.data_ptr(),
                                         ws.numel(), st())
        assert rc == 0, rc

    def class_grad_walk():
        rc = lib.hmm_class_posterior_grad_walk(A.data_ptr(), pi.data_ptr(), E.data_ptr(), *dims, engine.EPS,
                                               engine.POST_LOG, ctab, C, P.data_ptr(), Gc.data_ptr(), dA.data_ptr(),
                                               dpi.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel(), st())
        assert rc == 0, rc

    variants = (("composed", composed), ("fused", fused), ("posterior_walk", walk), ("class_posterior_walk", class_walk),
                ("posterior_grad_walk", grad_walk), ("class_posterior_grad_walk", class_grad_walk))
    for _, fn in variants:                                   # warm-up: workspaces, code objects, the allocator
        fn()
        fn()
    torch.cuda.synchronize()
    refused = lib.hmm_posterior_grad_walk_refused(*dims, ws.data_ptr(), ws.numel())
    assert refused == 0, refused
    times = {n: [] for n, _ in variants}
    for _ in range(rounds):
        for n, fn in variants:
            grads.clear()
            a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            z.record()
            z.synchronize()
            times[n].append(a.elapsed_time(z))
    for n, _ in variants:
        t = times[n]
        rec[n + "_ms"] = {"min": round(min(t), 4), "median": round(statistics.median(t), 4),
                          "spread": round(max(t) - min(t), 4)}
    med = lambda n: rec[n + "_ms"]["median"]                  # noqa: E731
    rec["composed_over_fused"] = round(med("composed") / med("fused"), 3)
    rec["walk_over_class_walk"] = round(med("posterior_walk") / med("class_posterior_walk"), 3)
    rec["grad_walk_over_class_grad_walk"] = round(med("posterior_grad_walk") / med("class_posterior_grad_walk"), 3)
    rec["peak_composed_over_fused"] = round(rec["composed_peak_bytes"] / rec["fused_peak_bytes"], 3)
    rec["pays"] = int(rec["composed_over_fused"] >= MARGIN)
    print(json.dumps(rec), flush=True)


def pays_table(path):
    """The step lines of a run -> {q: {b: ratios, peaks and pays}}."""
    recs = [json.loads(x) for x in open(path) if x.startswith("{")]
    out = {}
    for r in recs:
        out.setdefault(str(r["q"]), {})[str(r["b"])] = {
            "composed_ms": r["composed_ms"]["median"], "fused_ms": r["fused_ms"]["median"],
            "composed_over_fused": r["composed_over_fused"], "walk_over_class_walk": r["walk_over_class_walk"],
            "grad_walk_over_class_grad_walk": r["grad_walk_over_class_grad_walk"],
            "composed_peak_bytes": r["composed_peak_bytes"], "fused_peak_bytes": r["fused_peak_bytes"],
            "inputs_bytes": r["inputs_bytes"], "pays": r["pays"]}
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
