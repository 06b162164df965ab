"""What the fp64 oracle alone must show about the cases of tests/eps_cases.py before tests/test_eps_sweep_gpu.py runs
the kernels on them; no device needed.

  - every case is discriminating: between eps = 1e-16 and its own eps the fp64 posteriors or the fp64 log-likelihood
    move by at least ten of the tolerances the device is held to (gamma 2e-5, log-likelihood 1e-6 |ll| + 2e-4), the
    gradients by ten of the tensor norm's 3e-4.  A kernel that used the default anywhere misses by that much.  Blank
    rows and L = 1 move the log-likelihood only; every other case moves the posteriors as well;
  - the class-map decode cases leave the margin rule of tests/test_posterior_decode_gpu.py at most 1 % of the positions;
  - e32, the error of the fp32 restatement of the recursion, is far below the tolerances, so no case needs the
    conditioning rule to start with (eps_cases.CONDITIONED is empty unless the device says otherwise);
  - the table covers what it is for;
  - the C ABI refuses eps outside [HMM_EPS_MIN, HMM_EPS_MAX] in every entry point that takes eps.
"""
import re
import os

import numpy as np
import pytest

import eps_cases as ec
import posterior_decode_ref as dref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("spec", ec.posterior_cases() + ec.refusal_cases(), ids=ec.spec_id)
def test_case_is_discriminating(spec):
    g, ll = ec.moved(spec)
    e32 = [r["e32"] for r in ec.reference(spec)]
    print("EPS %s: the oracle moves by %.3g tolerances in gamma, %.3g in loglik; e32 gamma %.2e, loglik %.2e of its "
          "tolerance" % (ec.spec_id(spec), g, ll, max(e["gamma"] for e in e32), max(e["ll"] for e in e32)))
    assert max(g, ll) >= ec.DISCRIMINATING
    assert all(4 * e["gamma"] <= ec.TOL_GAMMA and 4 * e["ll"] <= 1.0 for e in e32)
    for r in ec.reference(spec):
        assert np.isfinite(r["gamma"]).all() and np.isfinite(r["ll"]).all()
        assert np.isfinite(r["la"]).all() and np.isfinite(r["lb"]).all()


@pytest.mark.parametrize("spec", ec.decode_cases(), ids=ec.spec_id)
def test_decode_margin(spec):
    table, C, n_max = ec.class_map(spec)
    assert len(table) == spec.q and max(table.count(c) for c in range(C)) == n_max
    for r in ec.reference(spec):
        sure = dref.decode(r["gamma"], table, C)[2] > ec.decode_margin_rule(n_max)
        print("EPS %s: %.4f of the positions outside the margin" % (ec.spec_id(spec), sure.mean()))
        assert sure.mean() >= 0.99


@pytest.mark.parametrize("g", ec.grad_cases(), ids=ec.gspec_id)
def test_grad_case_is_discriminating(g):
    mv = ec.grad_moved(g)
    ref = ec.grad_reference(g)
    print("EPS %s: the oracle's gradient moves by %.3g limits; e32 %s" % (
        ec.gspec_id(g), mv, {n: "%.1e" % max(r["e32"][n] for r in ref) for n in ref[0]["e32"]}))
    assert mv >= ec.DISCRIMINATING
    c, e = ec.build(g.spec), np.float32(g.spec.eps)
    for m, r in enumerate(ref):
        assert all(np.isfinite(x).all() for x in r["want"])
        assert all(lim <= 1e-3 for lim in r["limit"].values()), r["limit"]
        clamped = c["E"][m] <= e
        assert clamped.any() == (g.spec.emis != "plain")
        assert np.all(r["want"][2][clamped] == 0.0)                               # the oracle: no gradient there
    if g.spec.emis == "edge":
        E = c["E"]
        assert (E == e).any() and (E == np.nextafter(e, np.float32(0))).any() and (E == np.nextafter(e, np.float32(1))).any()


def test_the_handover_case_clamps_between_two_chunks_only():
    """eps_cases.HANDOVER: the reverse cell's clamp is active at one position of the whole call, the last one of a
    chunk, and the clamp-free recursion (tests/algo_model.py: the scan plan without its certificate) is then wrong by
    more than the tolerance before that position and right after it."""
    import algo_model
    s = ec.HANDOVER
    c, r, e = ec.build(s), ec.reference(s)[0], ec.eps32(s.eps)
    assert ec.backward_clamps(c["A"][0], c["pi"][0], c["E"][0], e) == [ec.HANDOVER_AT]
    seq, t = ec.HANDOVER_AT
    assert s.T == 16 and t % s.T == s.T - 1
    g = algo_model.posterior(c["A"][0], c["pi"][0], c["E"][0, seq], s.T, eps=e)[0]
    err = np.abs(g - r["gamma"][seq]).max(-1)
    print("EPS handover: the clamp-free scan is off by %.3g up to position %d, %.3g after it" % (
        err[:t + 1].max(), t, err[t + 1:].max()))
    assert err[:t + 1].max() >= 2 * ec.TOL_GAMMA and err[t + 1:].max() <= 0.1 * ec.TOL_GAMMA


@pytest.mark.parametrize("q", ec.HANDOVER_Q)
def test_the_constructed_handover_cases(q):
    """eps_cases.handover_case: one reverse clamp, at the last position of a chunk, no forward clamp; the clamp-free
    scan (tests/algo_model.py) is off by tens of tolerances before it and right after it."""
    import algo_model
    import postgrad_mid_cases as pm
    c, e, t = ec.handover_case(q), ec.eps32(ec.HANDOVER_EPS), ec.HANDOVER_POS
    A, pi, E = c["A"][0], c["pi"][0], c["E"][0]
    assert ec.backward_clamps(A, pi, E, e) == [(0, t)] and t % ec.HANDOVER_T == ec.HANDOVER_T - 1
    g64, count = pm.forward_backward64(A, pi, E, eps=e)
    assert count["forward"] == 0 and count["backward"] == 1 and count["pi"] == 0
    g = algo_model.posterior(A, pi, E[0], ec.HANDOVER_T, eps=e)[0]
    err = np.abs(g - g64[0]).max(-1)
    print("EPS handover q=%d: the clamp-free scan is off by %.3g up to position %d, %.3g after it" % (
        q, err[:t + 1].max(), t, err[t + 1:].max()))
    assert err[:t + 1].max() >= 10 * ec.TOL_GAMMA and err[t + 1:].max() <= 0.1 * ec.TOL_GAMMA


def test_the_table_covers_what_it_is_for():
    cases = ec.posterior_cases()
    assert {s.eps for s in cases} == {1e-10, 1e-6, 1e-3}
    assert {s.eps for s in ec.refusal_cases()} == {1e-20, 1e-30}
    assert all(s.emis == "blank" and ec.eps32(s.eps) < ec.EPS_MIN for s in ec.refusal_cases())
    assert all(ec.EPS_MIN <= ec.eps32(s.eps) <= ec.eps32(ec.EPS_MAX) for s in cases)
    assert {s.emis for s in cases} == {"plain", "rare", "zeros", "blank", "edge"}
    by = lambda name: {s.q for s in cases if name in s.models}
    assert by("gene") == {7, 15, 29, 43, 57} and by("gene-fd") == {15}
    assert {1, 2, 5, 13, 16, 17, 32, 33, 48, 64} <= by("dense")
    assert min(by("triu")) <= 16 < max(by("triu")) and min(by("thin")) <= 16 < max(by("thin"))
    assert any(len(s.models) == 2 for s in cases if s.q <= 16) and any(len(s.models) == 2 for s in cases if s.q > 16)
    assert {1, 17} <= {s.L for s in cases} and max(s.b for s in cases) <= 5
    for mid in (False, True):                                # 13 chunks, and more than 32 (the two-level scan)
        Ls = {s.L for s in cases if ec.is_mid(s) == mid and s.T == 16}
        assert 200 in Ls and 641 in Ls
    for s in cases:
        if "thin" in s.models:
            edge = float(ec.build(s)["A"][0, 0, s.q - 1])
            assert ec.eps32(ec.CONTROL) < edge < ec.eps32(s.eps)
    routes = {(g.route, g.spec.q > 16) for g in ec.grad_cases()}
    assert routes == {("chunk", False), ("whole", False), ("whole", True), ("scan", True)}
    assert {g.spec.q for g in ec.grad_cases() if g.route == "scan"} == {29, 43}


# ---- the domain of eps through the C ABI --------------------------------------------------------------------------
BAD_EPS = (0.0, -1e-16, float("nan"), float("inf"), 1e-20, 1e-30, 9.9e-19, 1.1e-3, 1.0)
GOOD_EPS = (1e-18, 1e-16, 1e-10, 1e-6, 1e-3)


@pytest.fixture(scope="module")
def lib():
    from hmm_layer_amd import build as hbuild
    from hmm_layer_amd import engine
    hbuild.build()
    return engine.lib()


def eps_entry_points():
    """{symbol: [(C type, parameter name), ...]} of every function of include/hmm_engine.h with a `float eps` parameter,
    from the header's own declarations."""
    text = open(os.path.join(ROOT, "include", "hmm_engine.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = {}
    for name, args in re.findall(r"\b(hmm_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", text):
        params = [re.match(r"(.*?)(\w+)$", " ".join(a.split())).groups() for a in args.split(",")]
        params = [(t.strip(), n) for t, n in params]
        if ("float", "eps") in params:
            out[name] = params
    return out


def test_the_header_states_the_domain():
    text = open(os.path.join(ROOT, "include", "hmm_engine.h")).read()
    assert float(re.search(r"#define HMM_EPS_MIN (\S+?)f\b", text).group(1)) == ec.EPS_MIN
    assert float(re.search(r"#define HMM_EPS_MAX (\S+?)f\b", text).group(1)) == ec.EPS_MAX


def test_every_entry_point_refuses_eps_outside_the_domain(lib):
    """Every function of the header that takes eps, called with plausible pointers (never dereferenced), a valid shape
    and a misaligned workspace, without a device: an eps outside the domain is HMM_ERR_BAD_ARGUMENT (-6); one inside it
    gets past the check and the call stops at the workspace (-4), before any HIP call."""
    import ctypes
    from hmm_layer_amd import engine
    points = eps_entry_points()
    assert len(points) >= 24 and {"hmm_forward", "hmm_backward", "hmm_posterior", "hmm_posterior_profiled",
                                  "hmm_posterior_decode", "hmm_posterior_decode_mid", "hmm_posterior_grad",
                                  "hmm_posterior_grad_scan", "hmm_loglik_grad", "hmm_loglik_grad_scan",
                                  "hmm_class_posterior", "hmm_class_posterior_grad", "hmm_seqshard_reduce",
                                  "hmm_seqshard_posterior", "hmm_seqshard_mid_reduce", "hmm_seqshard_mid_posterior",
                                  "hmm_posterior_walk", "hmm_loglik_grad_walk", "hmm_posterior_grad_walk",
                                  "hmm_loglik_grad_large", "hmm_posterior_grad_large"} <= set(points)
    raw = ctypes.CDLL(engine.LIB_PATH)
    p = 0x10000                                                                # never dereferenced
    table = (ctypes.c_int * 4096)()                                            # a class map read on the host: one class
    ctype = {"int": ctypes.c_int, "float": ctypes.c_float, "size_t": ctypes.c_size_t}
    # a valid call of every entry point: one model, two sequences (slabs) of 700 positions, rank 0 of 1, POST_PROB
    values = dict(k=1, b=2, L=700, Ls=700, seq_start=1, R=1, r=0, mode=0, num_classes=1, workspace_bytes=1 << 40,
                  workspace=p + 4, stream=None, profile=None, state_class=ctypes.cast(table, ctypes.c_void_p).value)
    served = {}
    for name, params in sorted(points.items()):
        fn = getattr(raw, name)
        fn.restype = ctypes.c_int
        fn.argtypes = [ctypes.c_void_p if "*" in t else ctype[t] for t, _ in params]
        at = params.index(("float", "eps"))
        for q in (15, 29, 100, 300):
            args = [q if n == "q" else values[n] if n in values else p if "*" in t else 0 for t, n in params]
            args[at] = 1e-16
            base = fn(*args)
            if base in (-1, -2):                                               # q outside this entry point's range
                continue
            assert base == -4, (name, q, base)
            for eps in BAD_EPS:
                args[at] = eps
                assert fn(*args) == -6, (name, q, eps)
            for eps in GOOD_EPS:
                args[at] = eps
                assert fn(*args) == -4, (name, q, eps)
            served.setdefault(name, []).append(q)
    assert set(served) == set(points), sorted(set(points) - set(served))
