"""What class posteriors cost for up to 16 states through the fused calls (hmm_class_posterior,
hmm_class_posterior_grad) next to the composition they replace, in time and in memory, and where
hmm_class_posterior_pays / hmm_class_posterior_grad_pays may say 1.

Per step (a model, a batch, a length), in ONE process: first the peak of torch.cuda.max_memory_allocated of one run of
each variant, each after the workspaces and the allocator's cache were released; then, after a warm-up of every variant,
timing with device events, the variants ALTERNATING round by round so that drift hits them alike; medians of 7 rounds.
Log mode, the upstream gradient of a mean cross-entropy against class labels: Gc = -one_hot(label) / (b L), the labels
uniform over the classes (`--labels random`, the profile's: most labels then sit on improbable classes, which the log
routing rule of hmm_class_posterior_grad hands to the whole-sequence sweeps) or each position's most probable class
(`--labels argmax`: nothing is exposed to the floors and the sequences stay per chunk).
  forward, composed   engine.posterior(POST_PROB) + engine.collapse_posterior + torch.log under no_grad: what
                      MsaHmmLayer.class_posterior_log_probs runs without the fused call
  forward, fused      engine.class_posterior(prob=False, log=True): what it runs with it
  node, composed      autograd.class_posterior(mode=POST_LOG, fused=False) + (Gc * .).sum().backward()
  node, fused         autograd.class_posterior(mode=POST_LOG, fused=True)  + (Gc * .).sum().backward()
The rule: a cell pays where median composed / median fused >= 1.25 (the margin of every _pays of the project);
`--table` folds the step lines of a run into profiles/class_posterior.json.  The fused node is compared with the
composed one on the same inputs: the largest difference of dA, dpi and dE (four sequences), each over the tensor's
largest entry.

Steps: the 7-state gene topology with 4 classes (intergenic and one per phase) and the 15-state gene model with 5, at
b x L = 1 x 100 000, 32 x 9 999, 1024 x 10 000 and 1024 x 100 000, emissions 0.05 + 0.9 u^4.  One child process per step
under its own time limit; the first failure stops the run.  One JSON line per step.

    python tools/experiments/class_posterior_time.py [--steps q15-32-9999,...] [--rounds N] [--labels random|argmax] [--out FILE]
    python tools/experiments/class_posterior_time.py --table FILE        the profile of the step lines in FILE
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
SHAPES = ((1, 100000), (32, 9999), (1024, 10000), (1024, 100000))
STEPS = tuple("q%d-%d-%d" % (q, b, L) for q in (7, 15) for b, L in SHAPES)
MARGIN = 1.25
CLASSES = {7: [0, 1, 2, 3, 1, 2, 3],                                   # Ir; intron and exon of a phase share a label
           15: [0, 1, 1, 1, 2, 3, 4, 2, 1, 1, 1, 1, 1, 1, 4]}           # the five labels of the 15-state gene model


def model(q):
    from oracle import params
    if q == 15:
        A = params.intended_A15(200, 4500, 10000)
    else:
        ed = params.edges_simple()
        A = params.dense_A(ed, params.init_logits(ed, 1, 200, 4500, 10000), 7)
    return A.float()[None].contiguous().to(DEV), torch.full((1, q), 1.0 / q, device=DEV)


def one(step, rounds, labels="random"):
    q, b, L = (int(x) for x in step[1:].split("-"))
    A, pi = model(q)
    table = CLASSES[q]
    C = max(table) + 1
    g = torch.Generator(device=DEV).manual_seed(7)
    E = torch.rand((1, b, L, q), device=DEV, generator=g).pow_(4).mul_(0.9).add_(0.05)
    if labels == "argmax":                                   # every label on its position's most probable class
        lab = engine.class_posterior(A, pi, E, table, C)[0].argmax(-1)
        engine.release_workspaces()
    else:                                                    # uniform over the classes, whatever their posterior
        lab = torch.randint(0, C, (1, b, L), device=DEV, generator=g)
    Gc = torch.zeros((1, b, L, C), device=DEV).scatter_(-1, lab[..., None], -1.0 / (b * L))
    del lab
    grads, keep = {}, {}

    def fwd_composed():
        with torch.no_grad():
            gamma = engine.posterior(A, pi, E, mode=engine.POST_PROB)[0]
            keep["fc"] = torch.log(engine.collapse_posterior(gamma, table, C))

    def fwd_fused():
        with torch.no_grad():
            keep["ff"] = engine.class_posterior(A, pi, E, table, C, prob=False, log=True)[1]

    def node(fused, name):
        leaves = [t.detach().requires_grad_(True) for t in (A, pi, E)]
        out = autograd.class_posterior(*leaves, table, C, mode=engine.POST_LOG, fused=fused)
        (Gc * out).sum().backward()
        grads[name] = [t.grad for t in leaves]

    variants = (("forward_composed", fwd_composed), ("forward_fused", fwd_fused),
                ("node_composed", lambda: node(False, "composed")), ("node_fused", lambda: node(True, "fused")))
    rec = {"step": step, "q": q, "b": b, "L": L, "rounds": rounds, "mode": "log", "classes": C, "G": "label", "labels": labels,
           "inputs_bytes": int(torch.cuda.memory_allocated())}
    # ---- memory first: one run each, from released workspaces and an empty cache
    for n, fn in variants:
        grads.clear()
        keep.clear()
        engine.release_workspaces()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        rec[n + "_peak_bytes"] = int(torch.cuda.max_memory_allocated())
    # the fused node against the composed one on the same inputs
    grads.clear()
    node(False, "composed")
    node(True, "fused")
    torch.cuda.synchronize()
    rec["fused_serial_sequences"] = engine.class_posterior_grad_serial_count((1, b, L, q))   # redone whole, of b
    big, got = grads["composed"], grads["fused"]
    rec["dA_max_rel_diff"] = float((got[0] - big[0]).abs().max() / big[0].abs().max())
    rec["dpi_max_rel_diff"] = float((got[1] - big[1]).abs().max() / big[1].abs().max())
    rec["dE_max_rel_diff"] = float((got[2][0, :min(b, 4)] - big[2][0, :min(b, 4)]).abs().max()
                                   / big[2][0, :min(b, 4)].abs().max())
    fwd_composed()
    fwd_fused()
    rec["forward_max_diff"] = float((keep["fc"][0, :min(b, 4)].exp() - keep["ff"][0, :min(b, 4)].exp()).abs().max())
    del big, got
    grads.clear()
    keep.clear()
    for _, fn in variants:                                   # warm-up: workspaces, code objects, the allocator
        fn()
        fn()
    torch.cuda.synchronize()
    times = {n: [] for n, _ in variants}
    for _ in range(rounds):
        for n, fn in variants:
            grads.clear()
            keep.clear()
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
    print(json.dumps(rec), flush=True)


def profile(path):
    """The step lines of a run -> the profile: per part (forward, node) one cell per step."""
    recs = [json.loads(x) for x in open(path) if x.startswith("{")]
    out = {"margin": MARGIN, "mode": "log", "G": "label", "labels": recs[0].get("labels", "random"),
           "rounds": recs[0]["rounds"], "forward": [], "node": []}
    for r in recs:
        for part in ("forward", "node"):
            c, f = r[part + "_composed_ms"]["median"], r[part + "_fused_ms"]["median"]
            cell = {"q": r["q"], "b": r["b"], "L": r["L"], "classes": r["classes"], "composed_ms": c, "fused_ms": f,
                    "composed_over_fused": round(c / f, 3), "composed_peak_bytes": r[part + "_composed_peak_bytes"],
                    "fused_peak_bytes": r[part + "_fused_peak_bytes"], "inputs_bytes": r["inputs_bytes"],
                    "pays": int(c / f >= MARGIN)}
            if part == "node":
                cell.update({n: r[n] for n in ("dA_max_rel_diff", "dpi_max_rel_diff", "dE_max_rel_diff", "fused_serial_sequences")
                             if n in r})
            else:
                cell["forward_max_diff"] = r["forward_max_diff"]
            out[part].append(cell)
    return out


def main():
    arg = lambda flag: sys.argv[sys.argv.index(flag) + 1] if flag in sys.argv else None   # noqa: E731
    if arg("--table"):
        print(json.dumps(profile(arg("--table")), indent=1))
        return
    rounds = int(arg("--rounds") or 7)
    labels = arg("--labels") or "random"
    if arg("--one"):
        return one(arg("--one"), rounds, labels)
    limit = int(arg("--limit") or 300)
    for step in (arg("--steps") or ",".join(STEPS)).split(","):
        # a child process per step, each under its own time limit; the first failure stops the run
        res = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", step, "--rounds", str(rounds), "--labels", labels],
                             capture_output=True, text=True, timeout=limit)
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
