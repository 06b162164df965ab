"""What the per-sequence walk for 65..256 states (hmm_posterior_walk, hmm_posterior_decode_wide) costs next to the
per-position GEMMs that hmm_posterior runs in this range, and where hmm_posterior_walk_pays may say 1.

Per step (a model, a batch), in ONE process, after a warm-up of every variant, timed with device events, the variants
ALTERNATING round by round so that drift hits them alike:
  (a)  engine.posterior(POST_PROB) into a kept tensor        the GEMM route, unchanged by the walk
  (a') engine.posterior_walk(POST_PROB)
  (b)  (a) + engine.decode_posterior                          what engine.posterior_decode composes above 64 states
  (c)  hmm_posterior_decode_wide through the C ABI, 6 classes (whatever hmm_posterior_walk_pays says)
Reported per variant: the fastest round, the median, the spread (slowest - fastest).  The rule: a cell pays where
median (b) / median (c) >= 1.25 (the margin of hmm_posterior_grad_scan_pays); `--table` folds the step lines of a run
into the table of profiles/posterior_walk.json.  (c)'s labels are compared with (b)'s and the mismatches counted with
the largest class-posterior gap among them (both sums are fp32 in different orders: only near-ties may differ).

Steps: the 71-, 127- and 253-state gene models (sparse step, 1 hub) and dense 96 and 128 states (the dense step with A
in registers) at b = 1, 32, 1024 x L = 10 000, emissions 0.05 + 0.9 u^4, classes i % 6 for the dense models.  One child
process per step under its own time limit; the first failure stops the run.  One JSON line per step.

    python tools/experiments/posterior_walk_time.py [--steps g71-32,...] [--rounds N] [--L 10000] [--out FILE]
    python tools/experiments/posterior_walk_time.py --table FILE        the pays table of the step lines in FILE
"""
import ctypes
import json
import os
import statistics
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from hmm_layer_amd import engine  # noqa: E402

DEV = "cuda:0"
STEPS = tuple("%s-%d" % (m, b) for m in ("g71", "g127", "g253", "d96", "d128") for b in (1, 32, 1024))
MARGIN = 1.25


def classes(name, q):
    return [0] + [1 + (i % 14) // 3 for i in range(q - 1)] if name[0] == "g" else [i % 6 for i in range(q)]


def model(name, q):
    if name[0] == "d":
        g = torch.Generator(device=DEV).manual_seed(q)
        A = torch.rand((1, q, q), device=DEV, generator=g) ** 3 + 1e-3
        return (A / A.sum(-1, keepdim=True)).contiguous(), torch.full((1, q), 1.0 / q, device=DEV)
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
    A, pi = model(name, q)
    g = torch.Generator(device=DEV).manual_seed(7)
    E = torch.rand((1, b, L, q), device=DEV, generator=g).pow_(4).mul_(0.9).add_(0.05)
    table, C = classes(name, q), 6
    ctab = (ctypes.c_int * q)(*table)
    lib = engine.lib()
    dims = (1, b, L, q)
    gamma = torch.empty_like(E)
    ws = torch.empty(lib.hmm_posterior_decode_wide_workspace_bytes(*dims), dtype=torch.uint8, device=DEV)
    label = torch.empty((1, b, L), dtype=torch.uint8, device=DEV)
    conf = torch.empty((1, b, L), dtype=torch.float32, device=DEV)
    ll = torch.empty((1, b), dtype=torch.float64, device=DEV)

    def va():
        return engine.posterior(A, pi, E, out=gamma)

    def vw():
        return engine.posterior_walk(A, pi, E, mode=engine.POST_PROB)

    def vb():
        gm, l2 = engine.posterior(A, pi, E, out=gamma)
        return (*engine.decode_posterior(gm, table, C), l2)

    def vc():
        rc = lib.hmm_posterior_decode_wide(A.data_ptr(), pi.data_ptr(), E.data_ptr(), *dims, engine.EPS, ctab, C,
                                           label.data_ptr(), conf.data_ptr(), ll.data_ptr(), ws.data_ptr(), ws.numel(),
                                           torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc
        return label, conf, ll

    variants = (("posterior_gemm", va), ("posterior_walk", vw), ("posterior_gemm_plus_torch_collapse", vb),
                ("posterior_decode_wide", vc))
    for _, fn in variants:                                   # warm-up: workspaces, code objects, the allocator
        fn()
        fn()
    torch.cuda.synchronize()
    times = {n: [] for n, _ in variants}
    for _ in range(rounds):
        for n, fn in variants:
            a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            z.record()
            z.synchronize()
            times[n].append(a.elapsed_time(z))
    rec = {"step": step, "q": q, "b": b, "L": L, "classes": C, "rounds": rounds,
           "step_kind": "sparse" if name[0] == "g" else "dense"}
    for n, _ in variants:
        t = times[n]
        rec[n + "_ms"] = {"min": round(min(t), 4), "median": round(statistics.median(t), 4),
                          "spread": round(max(t) - min(t), 4)}
    rec["walk_over_gemm"] = round(rec["posterior_gemm_ms"]["median"] / rec["posterior_walk_ms"]["median"], 3)
    rec["decode_over_composition"] = round(rec["posterior_gemm_plus_torch_collapse_ms"]["median"]
                                           / rec["posterior_decode_wide_ms"]["median"], 3)
    rec["pays"] = int(rec["decode_over_composition"] >= MARGIN)
    l2, c2, ll2 = vb()
    l2, c2 = l2.clone(), c2.clone()
    l3, c3, ll3 = vc()
    torch.cuda.synchronize()
    diff = l2 != l3
    rec["label_mismatches"] = int(diff.sum())
    rec["conf_max_abs_diff"] = float((c2 - c3).abs().max())
    rec["mismatch_max_conf_gap"] = float((c2 - c3).abs()[diff].max()) if bool(diff.any()) else 0.0
    rec["loglik_max_rel_diff"] = float(((ll2 - ll3).abs() / ll2.abs()).max())
    print(json.dumps(rec), flush=True)


def pays_table(path):
    """The step lines of a run -> {step kind: {q: {b: pays}}} with the ratios next to it."""
    recs = [json.loads(x) for x in open(path) if x.startswith("{")]
    out = {}
    for r in recs:
        out.setdefault(r["step_kind"], {}).setdefault(str(r["q"]), {})[str(r["b"])] = {
            "decode_over_composition": r["decode_over_composition"], "walk_over_gemm": r["walk_over_gemm"],
            "pays": r["pays"]}
    return out


def main():
    arg = lambda flag: sys.argv[sys.argv.index(flag) + 1] if flag in sys.argv else None
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
