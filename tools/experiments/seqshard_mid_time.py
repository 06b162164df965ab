"""Sequence-sharded posteriors for 17-64 states on ONE GPU: what the two local calls cost, ranks played in turn,
collectives not included (the method of seqshard_vscan_time.py).

For the 29- and 43-state gene models and a dense 48-state model, at b = 1 x L = 1e6 and b = 4 x L = 250 000:
  (a) engine.posterior (POST_LOG) on the whole tensor, at the same commit;
  (b) R = 8 equal slabs, each rank's own time for its reduce call and its posterior call (a stream and a workspace
      per rank), and per rank the kernels' own time by stage — reduce (the chunk operators), compose, hops (the scan
      over the R slab operators, the pick, the scan over the slab's chunks), apply (forward, backward, the rest) — from
      one more pass under torch.profiler.
Every figure of (a) and of the calls in (b) is the fastest of three passes after a warm-up, with a device
synchronisation around each call.  The sharded posteriors must agree with (a)'s to 1e-4 in probability.  One child
process per (model, shape), each under its own time limit; the first failure stops the run.  Prints one JSON line per
(model, shape); the projected ratio is (a) / max over ranks of (b): two real ranks, and the three collectives, are NOT
measured here.

    python tools/experiments/seqshard_mid_time.py [--models g29,g43,d48] [--out FILE] [--limit SECONDS]
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
R8, PASSES = 8, 3
STAGES = (("compose", "compose"), ("reduce", "reduce"), ("hops", "scan"), ("hops", "k_mid_pick"))


def model(name):
    """-> A (1,q,q), pi (1,q) on the device: gQ the gene model of (Q - 1) / 14 copies, dQ a dense model."""
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
    return A.float().reshape(1, q, q).contiguous(), pi.float().reshape(1, q).contiguous()


def emissions(b, L, q):
    g = torch.Generator(device=DEV).manual_seed(5)
    return torch.rand((1, b, L, q), device=DEV, generator=g) * 0.9 + 0.05


def timed(fn):
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
    if r not in _streams:
        _streams[r] = torch.cuda.Stream()
    return _streams[r]


def stage_of(kernel):
    for stage, word in STAGES:
        if word in kernel:
            return stage
    return "apply"


def sharded(A, pi, slabs, R, profile=False):
    """-> outs per rank, loglik, per-rank ms of (reduce call, posterior call) or, with profile, of the kernels by
    stage: every call timed on its own, ranks in turn."""
    from hmm_layer_amd import seqshard_mid as sm
    ms = [[0.0, 0.0] for _ in range(R)]
    split = [dict(reduce=0.0, compose=0.0, hops=0.0, apply=0.0) for _ in range(R)]

    def on(r, i, fn):
        def run():
            with torch.cuda.stream(rank_stream(r)):
                return fn()
        if not profile:
            ms[r][i], out = timed(run)
            return out
        from torch.profiler import ProfilerActivity, profile as prof
        torch.cuda.synchronize()
        with prof(activities=[ProfilerActivity.CUDA]) as p:
            out = run()
            torch.cuda.synchronize()
        for ev in p.events():
            if ev.device_type == torch.autograd.DeviceType.CUDA and "Memcpy" not in ev.name and "Memset" not in ev.name:
                us = ev.device_time if hasattr(ev, "device_time") else ev.cuda_time
                split[r][stage_of(ev.name)] += us / 1e3
        return out

    red = [on(r, 0, lambda: sm.reduce(A, slabs[r], r == 0, R)) for r in range(R)]
    all_ops = torch.stack([o for o, _ in red], dim=2).contiguous()
    all_exps = torch.stack([e for _, e in red], dim=2).contiguous()
    post = [on(r, 1, lambda: sm.posterior(A, pi, slabs[r], all_ops, all_exps, r, mode=engine.POST_LOG)) for r in range(R)]
    return [o for o, _, _ in post], post[0][1], (split if profile else ms), [p for _, _, p in post]


def one(name, b, L):
    """Child process: one (model, shape)."""
    A, pi = model(name)
    q = A.shape[-1]
    E = emissions(b, L, q)
    rec = {"model": name, "b": b, "L": L}
    whole_ms, (want, want_ll) = fastest(lambda: engine.posterior(A, pi, E, mode=engine.POST_LOG))
    rec["a_posterior_ms"] = round(whole_ms, 4)
    cuts = [L * r // R8 for r in range(R8 + 1)]
    slabs = [E[:, :, cuts[r]:cuts[r + 1]].contiguous() for r in range(R8)]
    best = None
    for i in range(PASSES + 1):                              # the first pass warms the workspaces up; keep the fastest
        outs, ll, ms, phis = sharded(A, pi, slabs, R8)
        if i == 0:
            err = max(float((torch.exp(outs[r]) - torch.exp(want[:, :, cuts[r]:cuts[r + 1]])).abs().max()) for r in range(R8))
            rec["max_abs_gamma_diff"] = err
            rec["phi_sum_max"] = float(sum(phis).max())
            rec["loglik_rel_diff"] = float(((ll - want_ll).abs() / want_ll.abs()).max())
            assert err <= 1e-4, "sharded posteriors differ from engine.posterior: %g" % err
        del outs
        if i and (best is None or max(sum(m) for m in ms) < max(sum(m) for m in best)):
            best = ms
    rec["R8_rank_ms"] = [round(sum(m), 4) for m in best]
    rec["R8_reduce_posterior_call_ms"] = [[round(x, 4) for x in m] for m in best]
    try:
        _, _, split, _ = sharded(A, pi, slabs, R8, profile=True)
        rec["R8_kernel_ms_by_stage"] = [{k: round(v, 4) for k, v in s.items()} for s in split]
    except Exception as e:                                   # the figures above stand without the split
        rec["R8_kernel_ms_by_stage"] = "unavailable: %s" % (str(e)[:120],)
    rec["projected_ratio_posterior_over_max_rank_R8"] = round(whole_ms / max(rec["R8_rank_ms"]), 3)
    rec["note"] = "one GPU, ranks in turn, collectives not included; two real ranks unmeasured"
    print(json.dumps(rec), flush=True)


def main():
    arg = lambda flag: sys.argv[sys.argv.index(flag) + 1] if flag in sys.argv else None
    if arg("--one"):
        name, b, L = arg("--one").split(",")
        return one(name, int(b), int(L))
    limit = int(arg("--limit") or 150)
    for name in (arg("--models") or "g29,g43,d48").split(","):
        for b, L in SHAPES:
            # a child process per step, each under its own time limit; the first failure stops the run
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", "%s,%d,%d" % (name, b, L)],
                                 capture_output=True, text=True, timeout=limit)
            if res.returncode != 0:
                print(res.stdout + res.stderr[-2000:], flush=True)
                sys.exit("step %s b=%d L=%d ended with status %d: stopping" % (name, b, L, res.returncode))
            line = [x for x in res.stdout.splitlines() if x.startswith("{")][-1]
            print(line, flush=True)
            if arg("--out"):
                with open(arg("--out"), "a") as fh:
                    fh.write(line + "\n")


if __name__ == "__main__":
    main()
