"""hmm_class_posterior_walk / hmm_class_posterior_grad_walk (class posteriors with analytic gradients, 65..256 states)
without a device: the argument checks of the C ABI in the order the header states, the workspace and pays queries, the
typed symbols, the wrappers' refusals, autograd.class_posterior's routing and its composed route against the fp64
oracle, the layer's CPU path; and, from the fp64 oracle and its fp32 twin alone, that every case of
tests/class_posterior_walk_cases.py can carry the comparison of tests/test_class_posterior_walk_gpu.py."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import class_posterior_walk_cases as cc
import posterior_decode_mid_cases as dm
import postgrad_mid_cases as pm
from hmm_layer_amd import autograd
from hmm_layer_amd import build as hbuild
from hmm_layer_amd import engine

SPECS = cc.all_specs() + cc.refused_cases()
PROFILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "class_posterior_walk.json")


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
    # shape, q outside 65..256, pointers (both outputs NULL included), the class table, then the workspace
    p = 0x10000                                                                 # never dereferenced
    eps, big = 1e-16, 1 << 40
    k, b, L, q = 2, 3, 17, 71
    f = lib.hmm_class_posterior_walk
    assert f(None, None, None, k, b, 0, q, eps, None, 99, None, None, None, None, 0, None) == -1
    assert f(None, None, None, 0, b, L, 257, eps, None, 99, None, None, None, None, 0, None) == -1
    for bad_q in (1, 16, 64, 257, 4096):
        assert f(None, None, None, k, b, L, bad_q, eps, None, 99, None, None, None, None, 0, None) == -2, bad_q
    good = table(q, 6)
    for hole in range(5):                                                       # A, pi, E, state_class, workspace
        a = [p, p, p, good, p]
        a[hole] = None
        assert f(a[0], a[1], a[2], k, b, L, q, eps, a[3], 99, p, p, None, a[4], 0, None) == -3, hole
    assert f(p, p, p, k, b, L, q, eps, good, 99, None, None, p, p, 0, None) == -3          # neither output
    for C in (0, -1, 17, 256):
        assert f(p, p, p, k, b, L, q, eps, good, C, p, None, None, p, 0, None) == -6, C
    for bad in (-1, 6, 1000):
        assert f(p, p, p, k, b, L, q, eps, table(q, 6, bad), 6, None, p, None, p, 0, None) == -6, bad
    need = lib.hmm_class_posterior_walk_workspace_bytes(k, b, L, q)
    for outs in ((p, None), (None, p), (p, p)):
        assert f(p, p, p, k, b, L, q, eps, good, 6, *outs, None, p, need - 1, None) == -4
        assert f(p, p, p, k, b, L, q, eps, good, 6, *outs, None, p + 1, big, None) == -4


def test_backward_validation_order_without_device(lib):
    # shape, q, mode, pointers (class_prob in log mode only), the class table, then the workspace
    p = 0x10000
    eps, big = 1e-16, 1 << 40
    k, b, L, q = 2, 3, 17, 71
    f = lib.hmm_class_posterior_grad_walk
    LOG, PROB, NO_LL = engine.POST_LOG, engine.POST_PROB, engine.POST_LOG_NO_LL
    none = (None,) * 8
    assert f(None, None, None, k, b, 0, q, eps, 7, None, 99, *none[:6], 0, None) == -1
    assert f(None, None, None, k, 0, L, 64, eps, 7, None, 99, *none[:6], 0, None) == -1
    for bad_q in (1, 16, 64, 257, 4096):
        assert f(None, None, None, k, b, L, bad_q, eps, 7, None, 99, *none[:6], 0, None) == -2, bad_q
    for bad_mode in (NO_LL, -1, 7):
        assert f(None, None, None, k, b, L, q, eps, bad_mode, None, 99, *none[:6], 0, None) == -6, bad_mode
    good = table(q, 6)
    need = lib.hmm_class_posterior_grad_walk_workspace_bytes(k, b, L, q, 6)
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
        for bad in (-1, 6):
            assert f(p, p, p, k, b, L, q, eps, mode, table(q, 6, bad), 6, p, p, p, p, p, p, 0, None) == -6, bad
        assert f(p, p, p, k, b, L, q, eps, mode, good, 6, p, p, p, p, p, p, need - 1, None) == -4
        assert f(p, p, p, k, b, L, q, eps, mode, good, 6, p, p, p, p, p, p + 1, big, None) == -4


def test_workspace_queries(lib):
    fwd, decode = lib.hmm_class_posterior_walk_workspace_bytes, lib.hmm_posterior_decode_wide_workspace_bytes
    bwd, state = lib.hmm_class_posterior_grad_walk_workspace_bytes, lib.hmm_posterior_grad_walk_workspace_bytes
    up = lambda n: (n + 255) // 256 * 256                                       # noqa: E731
    for k, b, L, q in ((1, 1, 1, 65), (2, 3, 17, 71), (1, 5, 333, 128), (1, 2, 300, 129), (2, 3, 530, 256),
                      (1, 1024, 1000, 253)):
        assert fwd(k, b, L, q) == decode(k, b, L, q) > 4 * k * b * L * q          # the parking region is included
        for C in (1, 6, 16):                                                    # the state call's layout first, then G'
            assert bwd(k, b, L, q, C) == state(k, b, L, q) + up(4 * k * b * L * C), (k, b, L, q, C)
        for C in (0, -1, 17):
            assert bwd(k, b, L, q, C) == 0
    for q in (1, 16, 64, 257, 1027):
        assert fwd(2, 3, 17, q) == 0 and bwd(2, 3, 17, q, 6) == 0, q
    for dims in ((0, 3, 17, 71), (2, 0, 17, 71), (2, 3, 0, 71)):
        assert fwd(*dims) == 0 and bwd(*dims, 6) == 0


def test_pays_is_zero_outside_the_range_and_follows_the_measurements(lib):
    for dims in ((1, 32, 10000, 64), (1, 32, 10000, 257), (0, 32, 10000, 71), (1, 32, 0, 71), (1, 0, 10, 127)):
        assert lib.hmm_class_posterior_walk_pays(*dims) == 0, dims
    with open(PROFILE) as fh:
        prof = json.load(fh)
    assert prof["margin"] == 1.25
    assert {(q, b) for q in prof["pays"] for b in prof["pays"][q]} == {(str(q), str(b)) for q in cc.GENE_Q for b in (1, 32, 1024)}
    paying = set()
    for q, cells in prof["pays"].items():
        for b, cell in cells.items():
            assert cell["pays"] == int(cell["composed_over_fused"] >= prof["margin"])
            assert cell["composed_over_fused"] == round(cell["composed_ms"] / cell["fused_ms"], 3)
            assert lib.hmm_class_posterior_walk_pays(1, int(b), prof["L"], int(q)) == cell["pays"], (q, b)
            assert cell["fused_peak_bytes"] < cell["composed_peak_bytes"]
            if cell["pays"]:
                paying.add((int(q), int(b)))
    assert paying                                                               # (else the predicate is a constant)
    # every cell that was not measured stays 0: other state counts, other numbers of sequences
    for q in (65, 70, 72, 128, 129, 252, 256):
        for k, b in ((1, 1), (1, 32), (1, 1024), (2, 512), (1, 4096)):
            assert lib.hmm_class_posterior_walk_pays(k, b, 10000, q) == 0, (k, b, q)
    for q in cc.GENE_Q:
        for k, b in ((1, 2), (1, 33), (1, 512), (1, 1023), (1, 1025), (2, 512), (2, 513), (4, 256), (1, 4096)):
            assert lib.hmm_class_posterior_walk_pays(k, b, 10000, q) == 0, (k, b, q)       # (one model was measured)
        for L in (1, 500, 100000):                          # L does not enter (the siblings' convention)
            assert lib.hmm_class_posterior_walk_pays(1, 1024, L, q) == int((q, 1024) in paying)


def test_symbols_are_typed(lib):
    assert set(engine.CLASS_POSTERIOR_WALK_SIGNATURES) == {
        "hmm_class_posterior_walk_workspace_bytes", "hmm_class_posterior_walk_pays", "hmm_class_posterior_walk",
        "hmm_class_posterior_grad_walk_workspace_bytes", "hmm_class_posterior_grad_walk"}
    for name, (restype, argtypes) in engine.CLASS_POSTERIOR_WALK_SIGNATURES.items():
        assert name not in engine._SIGNATURES and name not in engine.POSTERIOR_GRAD_WALK_SIGNATURES
        assert name not in engine.POSTERIOR_WALK_SIGNATURES
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes)
    tags = (engine.CLASS_WALK_TAG, engine.CLASS_GRAD_WALK_TAG, engine.POSTGRAD_WALK_TAG, engine.GRAD_WALK_TAG,
            engine.WALK_TAG, engine.DECODE_TAG)
    assert len(set(tags)) == len(tags)


def test_wrappers_refuse(lib):
    for q in (16, 64, 257, 1027):
        E = torch.rand(1, 2, 5, q)
        A, pi, tab = torch.eye(q)[None], torch.ones(q) / q, [0] * q
        with pytest.raises(ValueError, match="65..256"):
            engine.class_posterior_walk(A, pi, E, tab)
        with pytest.raises(ValueError, match="65..256"):
            engine.class_posterior_grad_walk(A, pi, E, tab, 1, torch.ones(1, 2, 5, 1), mode=engine.POST_PROB)
    q = 71
    A, pi, E = torch.eye(q)[None], torch.ones(q) / q, torch.rand(1, 2, 5, q)
    tab = dm.gene_classes(q)
    G = torch.ones(1, 2, 5, 6)
    with pytest.raises(ValueError, match="class table"):
        engine.class_posterior_walk(A, pi, E, None)
    with pytest.raises(ValueError, match="at most 16 classes"):
        engine.class_posterior_walk(A, pi, E, list(range(17)) + [0] * (q - 17))
    with pytest.raises(ValueError, match="0 .. num_classes-1"):
        engine.class_posterior_walk(A, pi, E, tab, 5)
    with pytest.raises(ValueError, match="q = 71 entries"):
        engine.class_posterior_walk(A, pi, E, tab[:-1])
    with pytest.raises(ValueError, match="prob, log or both"):
        engine.class_posterior_walk(A, pi, E, tab, prob=False, log=False)
    for mode in (engine.POST_LOG_NO_LL, 7):
        with pytest.raises(ValueError, match="POST_PROB or POST_LOG"):          # before the device is asked for
            engine.class_posterior_grad_walk(A, pi, E, tab, 6, G, class_prob=G, mode=mode)
    with pytest.raises(ValueError, match="needs class_prob"):
        engine.class_posterior_grad_walk(A, pi, E, tab, 6, G, mode=engine.POST_LOG)
    with pytest.raises(engine.EngineError, match="HIP device"):                 # in range: there is no CPU path
        engine.class_posterior_walk(A, pi, E, tab)
    with pytest.raises(engine.EngineError, match="HIP device"):
        engine.class_posterior_grad_walk(A, pi, E, tab, 6, G, class_prob=G)


def test_collapse_posterior_is_what_decode_posterior_sums():
    rng = np.random.default_rng(5)
    gamma = torch.tensor(rng.random((2, 3, 7, 29)), dtype=torch.float32)
    tab = dm.gene_classes(29)
    P = engine.collapse_posterior(gamma, tab, 6)
    want = torch.zeros(2, 3, 7, 6).index_add_(-1, torch.tensor(tab), gamma)
    assert torch.equal(P, want)
    label, conf = engine.decode_posterior(gamma, tab, 6)
    assert torch.equal(label, want.argmax(-1).to(torch.uint8)) and torch.equal(conf, want.max(-1).values)
    label, conf = engine.decode_posterior(gamma, None, 29)                      # the identity map sums nothing
    assert torch.equal(conf, gamma.max(-1).values)


def test_autograd_class_posterior_routing(lib, monkeypatch):
    q = 71
    A, pi, E = torch.eye(q)[None], torch.ones(q) / q, torch.rand(1, 2, 5, q)
    tab = dm.gene_classes(q)
    for bad in ("yes", 1.5, None, "True"):
        with pytest.raises(ValueError, match="support_only"):
            autograd.class_posterior(A, pi, E, tab, support_only=bad)
    with pytest.raises(ValueError, match="POST_PROB or POST_LOG"):
        autograd.class_posterior(A, pi, E, tab, mode=engine.POST_LOG_NO_LL)
    with pytest.raises(ValueError, match="class table"):
        autograd.class_posterior(A, pi, E, None)
    seen = []

    def composed(A, pi, E, mode=engine.POST_LOG, eps=engine.EPS, support_only=False):
        seen.append(("composed", int(mode), support_only))
        return E

    monkeypatch.setattr(autograd.ClassPosterior, "apply", lambda *a: seen.append(("fused", a[3], a[4], a[5])) or "F")
    monkeypatch.setattr(autograd, "posterior", composed)
    assert autograd.class_posterior(A, pi, E, tab, support_only="always") == "F"          # does not ask the predicate
    assert seen[-1] == ("fused", tab, 6, engine.POST_LOG)
    assert lib.hmm_class_posterior_walk_pays(1, 2, 5, q) == 0                             # as built: True composes
    for pays, want in ((1, "fused"), (0, "composed")):
        monkeypatch.setattr(lib, "hmm_class_posterior_walk_pays", lambda *dims, _v=pays: _v)
        autograd.class_posterior(A, pi, E, tab, support_only=True, mode=engine.POST_PROB)
        assert seen[-1][0] == want
    assert seen[-1] == ("composed", engine.POST_PROB, True)                               # state posteriors as probabilities
    out = autograd.class_posterior(A, pi, E, tab)
    assert seen[-1] == ("composed", engine.POST_PROB, False)
    assert torch.equal(out, torch.log(engine.collapse_posterior(E, tab, 6)))
    # more than 16 classes, or outside 65..256 states: composed, whatever support_only says
    monkeypatch.setattr(lib, "hmm_class_posterior_walk_pays", lambda *dims: 1)
    autograd.class_posterior(A, pi, E, list(range(17)) + [0] * (q - 17), support_only="always")
    assert seen[-1][0] == "composed"
    E29 = torch.rand(1, 2, 5, 29)
    out = autograd.class_posterior(torch.eye(29)[None], torch.ones(29) / 29, E29, dm.gene_classes(29),
                                   mode=engine.POST_PROB, support_only="always")
    assert seen[-1][0] == "composed" and torch.equal(out, engine.collapse_posterior(E29, dm.gene_classes(29), 6))


def test_composed_route_passes_nothing_through_a_class_of_posterior_zero(monkeypatch):
    """As the node (G' = 0 where P_c == 0): a non-empty class whose states all have posterior exactly 0 gives -inf in
    log mode and no gradient; torch.log alone would hand grad / 0 = inf to its states."""
    q, C = 71, 6
    tab = dm.gene_classes(q)
    dead = torch.tensor([c == 3 for c in tab])
    gamma = torch.rand(1, 2, 5, q, dtype=torch.float64)
    gamma[..., dead] = 0.0
    gamma = (gamma / gamma.sum(-1, keepdim=True)).requires_grad_(True)
    monkeypatch.setattr(autograd, "posterior", lambda A, pi, E, **kw: gamma)
    out = autograd.class_posterior(None, None, gamma, tab, C, mode=engine.POST_LOG)
    assert bool(torch.isneginf(out[..., 3]).all()) and bool(torch.isfinite(out[..., [0, 1, 2, 4, 5]]).all())
    out.backward(torch.ones_like(out))                                          # an upstream gradient for the dead class too
    assert bool(torch.isfinite(gamma.grad).all()) and bool((gamma.grad[..., dead] == 0).all())
    P = engine.collapse_posterior(gamma.detach(), tab, C)
    assert torch.allclose(gamma.grad[..., ~dead], (1 / P)[..., torch.tensor(tab)][..., ~dead])


@pytest.mark.parametrize("log", cc.MODES)
def test_composed_route_against_the_oracle(lib, monkeypatch, log):
    """autograd.class_posterior's torch ops (collapse, log) around a state posterior with autograd of its own — the
    fp64 recursion of oracle/torch64.py stands in for the engine's node, which needs a device — against the oracle:
    what is checked is the composition, the part of the route that runs without a device."""
    spec = cc.gene_sweep()[2 + int(log)]                                        # 71 states, rare, label
    assert (spec.q, spec.G, spec.log) == (71, "label", log)
    c, ref = cc.build(spec), cc.reference(spec)[0]
    tab, C = cc.table_of(spec)

    def host_posterior(A, pi, E, mode=engine.POST_LOG, eps=engine.EPS, support_only=False):
        assert int(mode) == engine.POST_PROB
        g = (pm.torch64.posterior(A[0], pi[0], E[0], eps)[0])[None]
        return g

    monkeypatch.setattr(autograd, "posterior", host_posterior)
    leaves = [torch.tensor(np.array(c[n]), dtype=torch.float64, requires_grad=True) for n in ("A", "pi", "E")]
    out = autograd.class_posterior(*leaves, list(tab), C, mode=engine.POST_LOG if log else engine.POST_PROB)
    assert out.shape == (1, spec.b, spec.L, C)
    G = torch.tensor(np.array(c["G"]), dtype=torch.float64)
    torch.where(G != 0, out * G, torch.zeros_like(out)).sum().backward()
    got = cc.on_support([leaves[0].grad[0].numpy(), leaves[1].grad[0].numpy(), leaves[2].grad[0].numpy()], c["A"][0])
    for g, w in zip(got, ref["want"]):
        assert np.abs(g - w).max() <= 1e-12 * max(np.abs(w).max(), 1.0)
    P = (torch.exp(out[0]) if log else out[0]).detach().numpy()
    assert np.abs(P - ref["P"]).max() <= 1e-12


def test_layer_cpu_path_against_the_oracle():
    """MsaHmmLayer.class_posterior_log_probs without gradients on the CPU (the step-at-a-time posterior, collapsed)
    for the five-copy model against the oracle's class sums."""
    from hmm_layer_amd.MsaHmmCell import HmmCell
    from hmm_layer_amd.MsaHMMLayer import MsaHmmLayer, _engine_inputs
    from hmm_layer_amd.gene_pred_hmm_emitter import GenePredHMMEmitter
    from hmm_layer_amd.gene_pred_hmm_transitioner import GenePredMultiHMMTransitioner
    from test_loglik_grad_large_gpu import CODONS
    b, L, q = 2, 40, 71
    g = torch.Generator().manual_seed(13)
    cls = torch.softmax(2 * torch.randn((1, b, L, 15), generator=g), -1)
    nuc = torch.nn.functional.one_hot(torch.randint(0, 4, (1, b, L), generator=g), 5).float()
    x = torch.cat([cls, nuc], -1)
    torch.manual_seed(5)
    np.random.seed(5)
    em = GenePredHMMEmitter(**CODONS, num_copies=5)
    em.build((1, b, L, 15))
    tr = GenePredMultiHMMTransitioner(k=5, initial_exon_len=200, initial_intron_len=4500, initial_ir_len=10000)
    cell = HmmCell([q], 15, em, tr)
    layer = MsaHmmLayer(cell, use_prior=False)
    layer.build(x.shape)
    tab = dm.gene_classes(q)
    with torch.no_grad():
        logp = layer.class_posterior_log_probs(x, tab)
        prob = layer.class_posterior_log_probs(x, torch.tensor(tab), 6, log=False)
        A, pi, E = _engine_inputs(x, cell, None, False)
    assert logp.shape == prob.shape == (1, b, L, 6) and logp.dtype == torch.float32
    gam, _ = pm.torch64.posterior(A[0].double(), pi[0].double(), E[0].double(), cell.epsilon)
    want = gam.numpy() @ cc.one_hot(tab, 6)
    assert np.abs(prob[0].numpy() - want).max() <= 1e-6                         # fp64 recursion, rounded to fp32 once
    assert np.abs(prob.sum(-1).numpy() - 1).max() <= 1e-6
    ok = want > 1e-30
    assert np.abs(logp[0].numpy() - np.log(np.where(ok, want, 1.0)))[ok].max() <= 1e-5 * np.abs(np.log(want[ok])).max() + 1e-6
    with pytest.raises(ValueError, match="class table"):
        layer.class_posterior_log_probs(x, None)


def test_posterior_decode_points_to_the_trainable_call():
    import inspect
    from hmm_layer_amd.MsaHMMLayer import MsaHmmLayer
    assert "class_posterior_log_probs" in inspect.getsource(MsaHmmLayer.posterior_decode)


@pytest.mark.parametrize("spec", SPECS, ids=cc.spec_id)
def test_case_can_carry_the_gpu_comparison(spec):
    c = cc.build(spec)
    table, C = cc.table_of(spec)
    k, b, L, q = c["E"].shape
    assert (k, q, b, L) == (len(spec.models), spec.q, spec.b, spec.L) and c["G"].shape == (k, b, L, C)
    assert all(c[n].dtype == np.float32 for n in ("A", "pi", "E", "G")) and c["A"].shape == (k, q, q)
    assert cc.Q_MIN <= q <= cc.Q_MAX and k * b <= 130 and L <= 300                # every GPU case is small
    assert len(table) == q and 1 <= C <= cc.MAX_CLASSES and min(table) >= 0 and max(table) < C
    used = np.bincount(np.asarray(table), minlength=C) > 0
    assert used.all() != (spec.table == "empty") and (spec.table != "empty" or not used[cc.EMPTY_CLASS])
    if spec.G == "label":                                                       # one class per position, never an empty one
        assert set(np.unique(c["G"])) <= {-1.0, 0.0} and np.all(c["G"].sum(-1) == -1.0)
        assert np.all(c["G"][..., ~used] == 0.0)
    if k == 2:
        assert not np.array_equal(c["A"][0], c["A"][1])
    assert cc.violations(spec) == []
    for m, ref in enumerate(cc.reference(spec)):
        A = c["A"][m]
        if ref is None:
            assert spec.models[m] == cc.REFUSED
            continue
        assert set(ref["limit"]) == set(cc.fine_norms(spec))
        assert cc.check(ref["want"], ref, A)[1]["tensor"] == 3e-4                # the tensor norm, whatever the table
        for n in cc.fine_norms(spec):
            assert ref["small"][n] <= 0.05 and 4 * ref["e32"][n] <= 1e-3, (m, n, ref["small"][n], ref["e32"][n])
            assert ref["limit"][n] == max(3e-4, 4 * ref["e32"][n])
        assert np.all(ref["want"][0][A == 0] == 0.0)                             # the reference on the support of A
        assert np.abs(ref["P"].sum(-1) - 1).max() <= 1e-12 and np.all(ref["P"][..., ~used] == 0.0)
        if spec.table == "one":                                                 # P = 1: nothing but rounding noise
            assert all(np.abs(w).max() <= 1e-9 for w in ref["want"])
            assert ref["e32"]["tensor"] <= 3e-4                                  # the twin itself within the tensor norm
        if spec.log:
            on = (c["G"][m] != 0) & used
            assert ref["P"][on].min() >= cc.MIN_P
        if L == 1:
            assert np.all(ref["want"][0] == 0.0)
        clampedE = c["E"][m] <= spec.eps
        assert np.all(ref["want"][2][clampedE] == 0.0) and np.all(ref["want"][1][c["pi"][m] <= spec.eps] == 0.0)


def test_the_oracle_is_the_state_level_oracle_with_the_expanded_gradient():
    """Prob mode: sum Gc P = sum G gamma with G[t][j] = Gc[t][class(j)] — the oracle of tests/postgrad_mid_cases.py on
    the expanded gradient gives the same derivative."""
    spec = cc.state_sweep()[0]._replace(log=False)
    c, ref = cc.build(spec), cc.reference(spec)[0]
    table, C = cc.table_of(spec)
    G = cc.expand(c["G"][0], table)
    assert G.shape == c["E"][0].shape and np.array_equal(G[..., 5], c["G"][0][..., table[5]])
    want = cc.on_support(pm.oracle(c["A"][0], c["pi"][0], c["E"][0], G, False, eps=spec.eps), c["A"][0])
    for g, w in zip(want, ref["want"]):
        assert np.abs(g - w).max() <= 1e-12 * max(np.abs(w).max(), 1.0)


def test_the_sweep_covers_what_it_is_for():
    specs = cc.all_specs()
    assert len({cc.spec_id(s) for s in specs}) == len(specs)
    assert set(cc.SEEDS) <= {cc.spec_id(s) for s in specs + cc.refused_cases()}             # no stale entry
    modes = {False, True}
    assert {(s.q, s.L, s.emis, s.G, s.log, s.table) for s in cc.gene_sweep()} == \
        {(q, L, e, G, log, "gene") for q in (71, 127, 253)
         for L, e, G in ((120, "holes", "dense"), (41, "rare", "label"), (41, "dead", "dense")) for log in modes}
    assert {(s.models[0], s.q, s.log) for s in cc.state_sweep()} == \
        {(kind, q, log) for q in (65, 96, 128, 129, 192, 193, 256) for kind in ("deg0", "deg1", "deg2") for log in modes}
    assert {s.table for s in cc.state_sweep()} == {"r2", "r5", "r16"} and {s.G for s in cc.state_sweep()} == {"dense", "label"}
    assert {(s.models[0], s.q, s.G, s.table) for s in cc.state_sweep()} >= \
        {("deg0", 65, "label", "r16"), ("deg1", 129, "label", "r16"), ("deg2", 256, "label", "r16")}
    assert all(s.L == 17 and s.b == 3 for s in cc.state_sweep())
    assert {(s.q, s.models, s.L, s.log) for s in cc.length_sweep()} == \
        {(q, ms, L, log) for q, ms in ((71, ("gene", "deg1")), (193, ("deg2", "deg0")))
         for L in (1, 2, 3, 7, 8, 9, 15, 16, 17, 33, 300) for log in modes}
    assert {(s.b, s.L, s.models, s.log) for s in cc.batch_sweep()} == \
        {(b, 24, ("gene", "deg2") if b < 130 else ("gene",), log) for b in (1, 3, 65, 130) for log in modes}
    assert all(s.eps == 1e-6 for s in cc.eps_cases()) and {s.eps for s in specs} == {1e-16, 1e-6}
    assert {s.table for s in cc.table_cases()} == {"empty", "one"}
    assert {cc.table_of(s)[1] for s in specs} == {1, 2, 5, 6, 16}
    assert all(s.models == ("deg3", "deg1") and s.q == 96 for s in cc.refused_cases())


def test_build_is_deterministic_and_read_only():
    s = cc.state_sweep()[0]
    a = cc.build(s)
    cc._build.cache_clear()
    b = cc.build(s)
    assert a is not b and all(np.array_equal(a[n], b[n]) for n in a)
    assert cc.build(s._replace(log=not s.log)) is b                             # both modes share their arrays
    with pytest.raises(ValueError):
        a["G"][0, 0, 0, 0] = 1.0
