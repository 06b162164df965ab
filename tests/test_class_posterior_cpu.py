"""hmm_class_posterior / hmm_class_posterior_grad (class posteriors with analytic gradients, up to 16 states) without a
device: the argument checks of the C ABI in the order the header states, the workspace and pays queries, the typed
symbols, the wrappers' refusals, autograd.class_posterior's `fused` routing; and, from the fp64 oracle and its fp32 twin
alone, that every case of tests/class_posterior_cases.py can carry the comparison of tests/test_class_posterior_gpu.py
and that the table covers the edges it is for."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import class_posterior_cases as cc
import postgrad_small_cases as ps
from hmm_layer_amd import autograd
from hmm_layer_amd import build as hbuild
from hmm_layer_amd import engine

SPECS = cc.all_specs()
PROFILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "class_posterior.json")


@pytest.fixture(scope="module")
def lib():
    hbuild.build()
    return engine.lib()


def table(q, C, bad=None):
    t = [i % C for i in range(q)]
    if bad is not None:
        t[q - 1] = bad
    return (ctypes.c_int * q)(*t)


def test_forward_validation_order_without_device(lib):
    # shape, q > 16, pointers (both outputs NULL included), the class table, then the workspace
    p = 0x10000                                                                 # never dereferenced
    eps, big = 1e-16, 1 << 40
    k, b, L, q = 2, 3, 17, 15
    f = lib.hmm_class_posterior
    assert f(None, None, None, k, b, 0, q, eps, None, 99, None, None, None, None, 0, None) == -1
    assert f(None, None, None, 0, b, L, 17, eps, None, 99, None, None, None, None, 0, None) == -1
    for bad_q in (17, 64, 65, 256, 4096):
        assert f(None, None, None, k, b, L, bad_q, eps, None, 99, None, None, None, None, 0, None) == -2, bad_q
    good = table(q, 5)
    for hole in range(5):                                                       # A, pi, E, state_class, workspace
        a = [p, p, p, good, p]
        a[hole] = None
        assert f(a[0], a[1], a[2], k, b, L, q, eps, a[3], 99, p, p, None, a[4], 0, None) == -3, hole
    assert f(p, p, p, k, b, L, q, eps, good, 99, None, None, p, p, 0, None) == -3          # neither output
    for C in (0, -1, 17, 256):
        assert f(p, p, p, k, b, L, q, eps, good, C, p, None, None, p, 0, None) == -6, C
    for bad in (-1, 5, 1000):
        assert f(p, p, p, k, b, L, q, eps, table(q, 5, bad), 5, None, p, None, p, 0, None) == -6, bad
    need = lib.hmm_class_posterior_workspace_bytes(k, b, L, q)
    for outs in ((p, None), (None, p), (p, p)):
        assert f(p, p, p, k, b, L, q, eps, good, 5, *outs, None, p, need - 1, None) == -4
        assert f(p, p, p, k, b, L, q, eps, good, 5, *outs, None, p + 1, big, None) == -4


def test_backward_validation_order_without_device(lib):
    # shape, q, mode, pointers (class_prob in log mode only), the class table, then the workspace
    p = 0x10000
    eps, big = 1e-16, 1 << 40
    k, b, L, q = 2, 3, 17, 15
    f = lib.hmm_class_posterior_grad
    LOG, PROB, NO_LL = engine.POST_LOG, engine.POST_PROB, engine.POST_LOG_NO_LL
    none = (None,) * 8
    assert f(None, None, None, k, b, 0, q, eps, 7, None, 99, *none[:6], 0, None) == -1
    assert f(None, None, None, k, 0, L, 64, eps, 7, None, 99, *none[:6], 0, None) == -1
    for bad_q in (17, 64, 65, 256, 4096):
        assert f(None, None, None, k, b, L, bad_q, eps, 7, None, 99, *none[:6], 0, None) == -2, bad_q
    for bad_mode in (NO_LL, -1, 7):
        assert f(None, None, None, k, b, L, q, eps, bad_mode, None, 99, *none[:6], 0, None) == -6, bad_mode
    good = table(q, 5)
    need = lib.hmm_class_posterior_grad_workspace_bytes(k, b, L, q, 5)
    for mode in (LOG, PROB):
        for hole in range(10):              # A, pi, E, state_class, class_prob, grad_out, dA, dpi, dE, workspace
            a = [p, p, p, good, p, p, p, p, p, p]
            a[hole] = None
            # class_prob is ignored in prob mode: the call goes on to the class table (99 classes)
            want = -6 if (hole == 4 and mode == PROB) else -3
            assert f(a[0], a[1], a[2], k, b, L, q, eps, mode, a[3], 99, a[4], a[5], a[6], a[7], a[8], a[9], 0,
                     None) == want, (mode, hole)
        for C in (0, -1, 17):
            assert f(p, p, p, k, b, L, q, eps, mode, good, C, p, p, p, p, p, p, 0, None) == -6, C
        for bad in (-1, 5):
            assert f(p, p, p, k, b, L, q, eps, mode, table(q, 5, bad), 5, p, p, p, p, p, p, 0, None) == -6, bad
        assert f(p, p, p, k, b, L, q, eps, mode, good, 5, p, p, p, p, p, p, need - 1, None) == -4
        assert f(p, p, p, k, b, L, q, eps, mode, good, 5, p, p, p, p, p, p + 1, big, None) == -4


def test_workspace_queries(lib):
    assert lib.hmm_class_posterior_max_states() == 16 == engine.CLASS_MAX_STATES
    fwd, bwd, state = (lib.hmm_class_posterior_workspace_bytes, lib.hmm_class_posterior_grad_workspace_bytes,
                       lib.hmm_posterior_grad_workspace_bytes)
    up = lambda n: (n + 255) // 256 * 256                                       # noqa: E731
    for k, b, L, q in ((1, 1, 1, 1), (2, 3, 17, 15), (1, 5, 333, 7), (1, 2, 3000, 16), (1, 32, 9999, 15),
                      (1, 1024, 1000, 15)):
        assert fwd(k, b, L, q) == lib.hmm_workspace_bytes(engine.OP_POSTERIOR, k, b, L, q) > 0
        sizes = [bwd(k, b, L, q, C) for C in (1, 5, 16)]
        # the state call's layout first, then G' (k b L C floats) and the rule's sums: at least both, growing with C
        for C, n in zip((1, 5, 16), sizes):
            assert n >= up(state(k, b, L, q)) + up(4 * k * b * L * C) and n % 256 == 0, (k, b, L, q, C)
        assert sizes[0] <= sizes[1] <= sizes[2] and (k * b * L < 64 or sizes[0] < sizes[1] < sizes[2])
        for C in (0, -1, 17):
            assert bwd(k, b, L, q, C) == 0
    for q in (17, 64, 65, 256, 1027):
        assert fwd(2, 3, 17, q) == 0 and bwd(2, 3, 17, q, 5) == 0, q
    for dims in ((0, 3, 17, 15), (2, 0, 17, 15), (2, 3, 0, 15), (2, 3, 17, 0)):
        assert fwd(*dims) == 0 and bwd(*dims, 5) == 0


def test_pays_is_zero_outside_the_range_and_follows_the_measurements(lib):
    for f in (lib.hmm_class_posterior_pays, lib.hmm_class_posterior_grad_pays):
        for dims in ((1, 32, 9999, 17), (1, 32, 9999, 64), (1, 1024, 10000, 71), (0, 32, 9999, 15), (1, 32, 0, 15),
                     (1, 0, 10, 15)):
            assert f(*dims) == 0, dims
    with open(PROFILE) as fh:
        prof = json.load(fh)
    assert prof["margin"] == 1.25
    want = {(q, b, L) for q in (7, 15) for b, L in ((1, 100000), (32, 9999), (1024, 10000), (1024, 100000))}
    for part, f in (("forward", lib.hmm_class_posterior_pays), ("node", lib.hmm_class_posterior_grad_pays)):
        cells = prof[part]
        assert {(c["q"], c["b"], c["L"]) for c in cells} == want
        for c in cells:
            assert c["classes"] == {7: 4, 15: 5}[c["q"]]
            ratio = c["composed_ms"] / c["fused_ms"]
            assert c["composed_over_fused"] == round(ratio, 3)
            assert c["pays"] == int(ratio >= prof["margin"]), c
            assert f(1, c["b"], c["L"], c["q"]) == c["pays"], c
            assert c["fused_peak_bytes"] > 0 and c["composed_peak_bytes"] > 0
            # everything not measured stays 0: neighbours of the cell in every coordinate, and two models
            for dims in ((1, c["b"] + 1, c["L"], c["q"]), (1, c["b"], c["L"] + 1, c["q"]), (1, c["b"], c["L"], c["q"] + 1),
                         (2, c["b"], c["L"], c["q"]), (1, c["b"], c["L"] - 1, c["q"])):
                if (dims[3], dims[1], dims[2]) not in want:
                    assert f(*dims) == 0, dims


def test_symbols_are_typed(lib):
    assert set(engine.CLASS_POSTERIOR_SIGNATURES) == {
        "hmm_class_posterior_max_states", "hmm_class_posterior_workspace_bytes", "hmm_class_posterior_pays",
        "hmm_class_posterior", "hmm_class_posterior_grad_workspace_bytes", "hmm_class_posterior_grad_pays",
        "hmm_class_posterior_grad"}
    others = (engine._SIGNATURES, engine.DECODE_SIGNATURES, engine.DECODE_MID_SIGNATURES, engine.POSTERIOR_WALK_SIGNATURES,
              engine.LOGLIK_GRAD_WALK_SIGNATURES, engine.POSTERIOR_GRAD_WALK_SIGNATURES,
              engine.CLASS_POSTERIOR_WALK_SIGNATURES)
    for name, (restype, argtypes) in engine.CLASS_POSTERIOR_SIGNATURES.items():
        assert not any(name in t for t in others), name
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes)
    tags = (engine.CLASS_TAG, engine.CLASS_GRAD_TAG, engine.CLASS_WALK_TAG, engine.CLASS_GRAD_WALK_TAG,
            engine.POSTGRAD_WALK_TAG, engine.GRAD_WALK_TAG, engine.WALK_TAG, engine.DECODE_TAG)
    assert len(set(tags)) == len(tags)


def test_wrappers_refuse(lib):
    for q in (17, 64, 65, 256):
        E = torch.rand(1, 2, 5, q)
        A, pi, tab = torch.eye(q)[None], torch.ones(q) / q, [0] * q
        with pytest.raises(ValueError, match="1..16 states"):
            engine.class_posterior(A, pi, E, tab)
        with pytest.raises(ValueError, match="1..16 states"):
            engine.class_posterior_grad(A, pi, E, tab, 1, torch.ones(1, 2, 5, 1), mode=engine.POST_PROB)
    q = 15
    A, pi, E = torch.eye(q)[None], torch.ones(q) / q, torch.rand(1, 2, 5, q)
    tab = [i % 5 for i in range(q)]
    G = torch.ones(1, 2, 5, 5)
    with pytest.raises(ValueError, match="class table"):
        engine.class_posterior(A, pi, E, None)
    with pytest.raises(ValueError, match="class table"):
        engine.class_posterior_grad(A, pi, E, None, 5, G)
    with pytest.raises(ValueError, match="at most 16 classes"):
        engine.class_posterior(A, pi, E, tab, 17)
    with pytest.raises(ValueError, match="0 .. num_classes-1"):
        engine.class_posterior(A, pi, E, tab, 4)
    with pytest.raises(ValueError, match="q = 15 entries"):
        engine.class_posterior(A, pi, E, tab[:-1])
    with pytest.raises(ValueError, match="prob, log or both"):
        engine.class_posterior(A, pi, E, tab, prob=False, log=False)
    for mode in (engine.POST_LOG_NO_LL, 7):
        with pytest.raises(ValueError, match="POST_PROB or POST_LOG"):          # before the device is asked for
            engine.class_posterior_grad(A, pi, E, tab, 5, G, class_prob=G, mode=mode)
    with pytest.raises(ValueError, match="needs class_prob"):
        engine.class_posterior_grad(A, pi, E, tab, 5, G, mode=engine.POST_LOG)
    with pytest.raises(engine.EngineError, match="HIP device"):                 # in range: there is no CPU path
        engine.class_posterior(A, pi, E, tab)
    with pytest.raises(engine.EngineError, match="HIP device"):
        engine.class_posterior_grad(A, pi, E, tab, 5, G, class_prob=G)


class FakeDevice(torch.Tensor):
    """A CPU tensor that says it lives on a HIP device: the routing reads E.is_cuda and nothing else of the device."""
    is_cuda = True


def test_autograd_class_posterior_fused_routing(lib, monkeypatch):
    q = 15
    A, pi, E = torch.eye(q)[None], torch.ones(q) / q, torch.rand(1, 2, 5, q)
    Ed = E.as_subclass(FakeDevice)
    tab = [i % 5 for i in range(q)]
    seen = []

    def composed(A, pi, E, mode=engine.POST_LOG, eps=engine.EPS, support_only=False):
        seen.append(("composed", int(mode), support_only))
        return E.as_subclass(torch.Tensor)

    monkeypatch.setattr(autograd.ClassPosteriorSmall, "apply", lambda *a: seen.append(("fused", a[3], a[4], a[5])) or "F")
    monkeypatch.setattr(autograd, "posterior", composed)
    for bad in ("yes", 1.5, "always", 2):
        with pytest.raises(ValueError, match="fused"):
            autograd.class_posterior(A, pi, Ed, tab, fused=bad)
    assert lib.hmm_class_posterior_grad_pays(1, 2, 5, q) == 0                   # as built: None composes on this shape
    out = autograd.class_posterior(A, pi, Ed, tab)
    assert seen[-1] == ("composed", engine.POST_PROB, False)
    assert torch.equal(out, torch.log(engine.collapse_posterior(E, tab, 5)))
    for pays, want in ((1, "fused"), (0, "composed")):                          # None asks the predicate
        monkeypatch.setattr(lib, "hmm_class_posterior_grad_pays", lambda *dims, _v=pays: _v)
        autograd.class_posterior(A, pi, Ed, tab, mode=engine.POST_PROB)
        assert seen[-1][0] == want
    assert autograd.class_posterior(A, pi, Ed, tab, fused=True) == "F"          # True does not ask
    assert seen[-1] == ("fused", tab, 5, engine.POST_LOG)
    monkeypatch.setattr(lib, "hmm_class_posterior_grad_pays", lambda *dims: 1)
    autograd.class_posterior(A, pi, Ed, tab, fused=False)                       # False composes whatever it says
    assert seen[-1][0] == "composed"
    # 17 classes, 17 states, a CPU tensor: composed under None, ValueError under True
    tab17 = list(range(15))
    for args in ((A, pi, Ed, tab17, 17), (torch.eye(17)[None], torch.ones(17) / 17, torch.rand(1, 2, 5, 17).as_subclass(FakeDevice),
                                          [0] * 17, 1), (A, pi, E, tab, 5)):
        n = len(seen)
        autograd.class_posterior(*args)
        assert [s[0] for s in seen[n:]] == ["composed"]
        with pytest.raises(ValueError, match="fused=True"):
            autograd.class_posterior(*args, fused=True)
    # the other routes of the function are as they were: support_only is validated and handed on
    with pytest.raises(ValueError, match="support_only"):
        autograd.class_posterior(A, pi, E, tab, support_only="yes")
    autograd.class_posterior(A, pi, E, tab, support_only=True, fused=False)
    assert seen[-1] == ("composed", engine.POST_PROB, True)


@pytest.mark.parametrize("spec", SPECS, ids=cc.spec_id)
def test_case_is_fit(spec):
    """From the oracle and its twin alone: the twin stays within the limits the engine will be held to, and the
    conditions of the case table's docstring hold."""
    assert cc.violations(spec) == []
    c = cc.build(spec)
    for m, ref in enumerate(cc.reference(spec)):
        if ref["absolute"] is not None:
            assert all(np.abs(w).max() <= 1e-12 for w in ref["want"])            # the truth is zero (to fp64 rounding)
            continue
        assert ref["e32"]["tensor"] <= cc.TENSOR_REL, (m, ref["e32"])
        for n in ref["norms"]:
            assert ref["e32"][n] <= ref["limit"][n]
    for r in cc.routing(spec):
        assert set(r["verdict"]) <= {"chunk", "whole", "open"}
    assert c["G"].shape == c["E"].shape[:3] + (cc.table_of(spec)[1],)


def test_table_covers_the_edges():
    ids = [cc.spec_id(s) for s in SPECS]
    assert len(set(ids)) == len(ids)
    assert {s.q for s in SPECS} == set(cc.STATES) == {1, 2, 7, 15, 16}
    assert {cc.table_of(s)[1] for s in SPECS} >= {1, 2, 5, 16}
    assert {s.L for s in SPECS} >= {1, 2, 3, 15, 16, 17, 33, 100, 300}
    assert {s.T for s in SPECS} == {0, 16, 48}
    assert {s.b for s in SPECS} >= {1, 3, 5, 130}
    assert {s.eps for s in SPECS} == {1e-16, 1e-6}
    assert {s.G for s in SPECS} == {"dense", "label", "labelx"} and {s.log for s in SPECS} == {False, True}
    assert {s.emis for s in SPECS} == {"plain", "holes", "rare", "dead", "clamp", "stretch"}
    names = {n for s in SPECS for n in s.models}
    assert names >= {"gene", "simple7", "shipped", "dense", "sparse", "triu", "dense-d", "sparse-d"}
    assert any(len(s.models) == 2 and s.models[0] != s.models[1] for s in SPECS)
    tables = {s.table for s in SPECS}
    assert tables >= {"one", "id", "empty", "gene", "r2", "r5", "r16"}
    assert any(cc.table_of(s)[1] > s.q for s in SPECS)                          # more classes than states
    for log in cc.MODES:                                                        # a gradient on an empty class
        assert any(s.table == "empty" and s.log == log and np.all(cc.build(s)["G"][..., cc.EMPTY_CLASS] != 0) for s in SPECS)
    # ragged rows: the number of chunks is no multiple of the four chunks a wave holds
    assert any((len(s.models) * s.b * ps.chunks(cc.state_spec(s))) % 4 for s in SPECS if cc.shipped_per_chunk(s))
    # both routing verdicts occur among the cases the shipped routing serves per chunk, in log mode too
    per_chunk = [s for s in SPECS if cc.shipped_per_chunk(s)]
    verdicts = {(s.log, v) for s in per_chunk for r in cc.routing(s) for v in r["verdict"]}
    assert {(False, "chunk"), (False, "whole"), (True, "chunk"), (True, "whole")} <= verdicts
    # ... and the class rule itself decides one of them: a sequence that the certificate alone would leave per chunk
    assert any(r["primitive"] and f / ps.EXACT_DELTA <= 1 / ps.MARGIN and v == "whole"
               for s in per_chunk if s.log for r in cc.routing(s) for f, v in zip(r["F"], r["verdict"]))
    assert any(cc.forced_per_chunk(s) for s in SPECS if s.log) and any(cc.forced_per_chunk(s) for s in SPECS if not s.log)
