"""What fused posterior decoding (engine.posterior_decode, up to 64 states) costs next to what users run today.

Per step (a model, a shape, a kind of input), in ONE process, after a warm-up of every variant, timed with device
events, the three variants ALTERNATING round by round so that drift hits them alike:
  (i)   engine.posterior(POST_PROB) alone                      writes gamma (k,b,L,q) fp32; like (iii) it allocates its
                                                               outputs per call ((i') = the same into a kept tensor)
  (ii)  (i) + the torch collapse users run today                index_add_ over the class axis, max, argmax
  (iii) engine.posterior_decode with the class map             writes 1 + 4 bytes per position
Reported per variant: the fastest round, the median, and the spread (slowest - fastest) — a difference between two
variants means something only against the spread of (i).  One more pass of (i) and (iii) under torch.profiler gives the
per-kernel split (tracing slows the host: those figures are kernel times, not call times).  The labels of (iii) are
compared with (ii)'s; positions where they differ are counted and the largest class-posterior gap among them is
reported (both sums are fp32, in different orders: only near-ties may differ).

Steps: the 15-state gene model at b = 1024 x L = 100 000 on uniform-random emissions and on the fused emitter's
output for softmax(2 randn) class probabilities (47 % zeros; the record says how many sequences were routed), at
b = 32 x L = 9999, and the 7-state model at b = 1024 x L = 100 000.  For 17..64 states (hmm_posterior_decode_mid;
MID_STEPS, emissions 0.05 + 0.9 u^4): the 29-state two-copy gene model onto 6 classes at b = 1024 x L = 100 000 and
b = 32 x L = 9999, the 43-state three-copy model at b = 1024 x L = 10 000 (every sequence on the one-wave-per-sequence
walk) and b = 32 x L = 9999 (the 64-lane scan), and a dense 24-state model at b = 128 x L = 100 000.  (ii) is timed on
the code path of the build before the fused kernels, engine.posterior + engine.decode_posterior.  One child process
per step under its own time limit; the first failure stops the run.  One JSON line per step.

    python tools/experiments/posterior_decode_time.py [--steps g15-1024-100000-uniform,...] [--rounds N] [--out FILE]
                                                      [--lib OTHER_BUILD.so]      (A/B of a kernel change)
    python tools/experiments/posterior_decode_time.py --calls STEP     three calls of (i) and of (iii), nothing timed and no
                                                                       child process: the program a profiler runs
"""
import json
import os
import statistics
import subprocess
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from hmm_layer_amd import engine  # noqa: E402

if "--lib" in sys.argv:                                      # another build of the engine
    engine.LIB_PATH = os.path.abspath(sys.argv[sys.argv.index("--lib") + 1])
DEV = "cuda:0"
STEPS = ("g15-1024-100000-uniform", "g15-1024-100000-emitter", "g15-32-9999-uniform", "g7-1024-100000-uniform")
MID_STEPS = ("g29-1024-100000-peaked", "g29-32-9999-peaked", "g43-1024-10000-peaked", "g43-32-9999-peaked",
             "d24-128-100000-peaked")                         # --steps mid
# Ir, I0-2, E0-2, START, EI0-2, IE0-2, STOP -> intergenic / intron / exon phase 0, 1, 2
CLASSES = {15: [0, 1, 1, 1, 2, 3, 4, 2, 1, 1, 1, 1, 1, 1, 4], 7: [0, 1, 1, 1, 2, 3, 4],
           # the multi-copy gene models: intergenic, then five classes per copy's 14 states, shared by the copies
           29: [0] + [1 + (i % 14) // 3 for i in range(28)], 43: [0] + [1 + (i % 14) // 3 for i in range(42)],
           24: [i % 6 for i in range(24)]}
CODONS = dict(start_codons=[("ATG", 1.)], stop_codons=[("TAG", .34), ("TAA", .33), ("TGA", .33)],
              intron_begin_pattern=[("NGT", .99), ("NGC", .005), ("NAT", .005)],
              intron_end_pattern=[("AGN", .99), ("ACN", .01)])


def model(q, dense=False):
    from hmm_layer_amd.gene_pred_hmm_transitioner import GenePredMultiHMMTransitioner, SimpleGenePredHMMTransitioner
    if dense:
        g = torch.Generator(device=DEV).manual_seed(q)
        A = torch.rand((1, q, q), device=DEV, generator=g) ** 3 + 1e-3
        return (A / A.sum(-1, keepdim=True)).contiguous(), torch.full((1, q), 1.0 / q, device=DEV)
    kw = dict(initial_exon_len=200, initial_intron_len=4500, initial_ir_len=10000, starting_distribution_init="zeros")
    tr = (SimpleGenePredHMMTransitioner(**kw) if q == 7 else GenePredMultiHMMTransitioner(k=(q - 1) // 14, **kw)).to(DEV)
    with torch.no_grad():
        A, pi = tr.make_A().contiguous(), tr.make_initial_distribution().reshape(1, -1).contiguous()
    assert A.shape[-1] == q
    return A.float(), pi.float()


def emissions(kind, b, L, q):
    g = torch.Generator(device=DEV).manual_seed(7)
    if kind == "uniform":
        return torch.rand((1, b, L, q), device=DEV, generator=g) * 0.9 + 0.05
    if kind == "peaked":
        return torch.rand((1, b, L, q), device=DEV, generator=g).pow_(4).mul_(0.9).add_(0.05)
    assert q == 15
    from hmm_layer_amd.gene_pred_hmm_emitter import GenePredHMMEmitter
    em = GenePredHMMEmitter(**CODONS)
    em.build((1, b, L, 15))
    with torch.no_grad():
        em.emission_kernel.copy_(torch.randn(em.emission_kernel.shape, generator=torch.Generator().manual_seed(0)))
    em = em.to(DEV)
    em.recurrent_init()
    x = torch.empty((1, b, L, 20), device=DEV)
    x[..., :15] = torch.softmax(2.0 * torch.randn((1, b, L, 15), device=DEV, generator=g), -1)
    idx = torch.where(torch.rand((1, b, L), device=DEV, generator=g) < 0.01, torch.full((1, b, L), 4, device=DEV),
                      torch.randint(0, 4, (1, b, L), device=DEV, generator=g))
    x[..., 15:] = torch.nn.functional.one_hot(idx, 5).float()
    del idx
    return em.forward_fused(x).contiguous()


def kernel_split(fn, passes=3):
    """Kernel time by kernel name (template arguments kept, parameter lists cut) of one call under torch.profiler:
    per kernel the fastest of `passes` calls."""
    from torch.profiler import ProfilerActivity, profile
    best = {}
    for _ in range(passes):
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as p:
            fn()
            torch.cuda.synchronize()
        out = {}
        for ev in p.events():
            if ev.device_type == torch.autograd.DeviceType.CUDA and "Memcpy" not in ev.name and "Memset" not in ev.name:
                us = ev.device_time if hasattr(ev, "device_time") else ev.cuda_time
                name = ev.name.split("(")[0].replace("void ", "")
                out[name] = out.get(name, 0.0) + us / 1e3
        best = {n: round(min(ms, best.get(n, ms)), 4) for n, ms in out.items()}
    return best


def calls(step):
    name, b, L, kind = step.split("-")
    q = int(name[1:])
    A, pi = model(q, name[0] == "d")
    E = emissions(kind, int(b), int(L), q)
    for _ in range(3):
        engine.posterior(A, pi, E)
        engine.posterior_decode(A, pi, E, CLASSES[q])
    torch.cuda.synchronize()
    print("done")


def one(step, rounds):
    name, b, L, kind = step.split("-")
    q, b, L = int(name[1:]), int(b), int(L)
    A, pi = model(q, name[0] == "d")
    E = emissions(kind, b, L, q)
    table, C = CLASSES[q], max(CLASSES[q]) + 1
    gamma = torch.empty_like(E)

    def v1():
        return engine.posterior(A, pi, E)

    def v1_out():
        return engine.posterior(A, pi, E, out=gamma)

    def v2():
        g, ll = engine.posterior(A, pi, E, out=gamma)
        return (*engine.decode_posterior(g, table, C), ll)

    def v3():
        return engine.posterior_decode(A, pi, E, table, C)

    variants = (("posterior", v1), ("posterior_into_kept_tensor", v1_out), ("posterior_plus_torch_collapse", v2),
                ("posterior_decode", v3))
    for _, fn in variants:                                   # warm-up: workspaces, code objects, the allocator
        fn()
        fn()
    torch.cuda.synchronize()
    times = {n: [] for n, _ in variants}
    host = {n: [] for n, _ in variants}                      # how long the host takes to enqueue the call
    for _ in range(rounds):
        for n, fn in variants:
            a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            a.record()
            fn()
            z.record()
            host[n].append((time.perf_counter() - t0) * 1e3)
            z.synchronize()
            times[n].append(a.elapsed_time(z))
    rec = {"lib": os.path.basename(engine.LIB_PATH), "step": step, "q": q, "b": b, "L": L, "input": kind, "classes": C, "rounds": rounds,
           "zero_emissions_fraction": round(float((E == 0).float().mean()), 4)}
    for n, _ in variants:
        t = times[n]
        rec[n + "_ms"] = {"min": round(min(t), 4), "median": round(statistics.median(t), 4),
                          "spread": round(max(t) - min(t), 4), "host_enqueue_median": round(statistics.median(host[n]), 4)}
    if q <= 16:
        rec["routing_decode"] = engine.exact_detail((1, b, L, q), tag=engine.DECODE_TAG)
        rec["routing_posterior"] = engine.exact_detail((1, b, L, q))
    else:       # sequences the walk served next to the chunked scan (0 where the walk serves the whole call by plan)
        rec["routing_decode"] = {"routed": engine.exact_count(engine.OP_POSTERIOR, (1, b, L, q), tag=engine.DECODE_TAG)}
        rec["routing_posterior"] = {"routed": engine.exact_count(engine.OP_POSTERIOR, (1, b, L, q))}
    # what the fused call returns against the composed one
    l2, c2, ll2 = v2()
    l3, c3, ll3 = v3()
    torch.cuda.synchronize()
    diff = l2 != l3
    rec["label_mismatches"] = int(diff.sum())
    rec["conf_max_abs_diff"] = float((c2 - c3).abs().max())
    rec["mismatch_max_conf_gap"] = float((c2 - c3).abs()[diff].max()) if bool(diff.any()) else 0.0
    rec["loglik_equal"] = bool(torch.equal(ll2, ll3))
    del l2, c2, l3, c3
    pos = float(b) * L
    rec["output_bytes_per_position"] = {"posterior": 4 * q, "posterior_decode": 5}
    rec["posterior_decode_positions_per_s"] = round(pos / (rec["posterior_decode_ms"]["min"] * 1e-3), 1)
    try:
        rec["kernel_ms_posterior"] = kernel_split(v1)
        rec["kernel_ms_posterior_decode"] = kernel_split(v3)
    except Exception as e:                                   # the figures above stand without the split
        rec["kernel_ms_posterior_decode"] = "unavailable: %s" % (str(e)[:120],)
    print(json.dumps(rec), flush=True)


def main():
    arg = lambda flag: sys.argv[sys.argv.index(flag) + 1] if flag in sys.argv else None
    rounds = int(arg("--rounds") or 30)
    if arg("--one"):
        return one(arg("--one"), rounds)
    if arg("--calls"):
        return calls(arg("--calls"))
    steps = arg("--steps") or ",".join(STEPS)
    # the 17..64-state steps hold E, two gamma tensors and a gamma-sized parking region (11.9 GB each at the largest)
    # and draw up to 3e9 emissions: a longer limit per child than the 15-state steps have
    limit = int(arg("--limit") or (300 if steps == "mid" else 150))
    for step in (",".join(MID_STEPS) if steps == "mid" else steps).split(","):
        # a child process per step, each under its own time limit; the first failure stops the run
        res = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", step, "--rounds", str(rounds)] +
                             (["--lib", engine.LIB_PATH] if arg("--lib") else []),
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
