"""hmm_posterior_grad_walk (posterior gradients by the per-sequence walk with the sparse step, 65..256 states) without
a device: the argument checks of the C ABI in the order the header states, the state, workspace and pays queries, the
typed symbols, the wrappers' refusals, autograd.posterior's support_only argument, the layer passing its
transitioner's flag; and, from the fp64 oracle and its fp32 twin alone, that every case of
tests/posterior_grad_walk_cases.py can carry the comparison of tests/test_posterior_grad_walk_gpu.py."""
import json
import os

import numpy as np
import pytest
import torch

import loglik_grad_cases as lc
import posterior_grad_walk_cases as pc
from hmm_layer_amd import autograd
from hmm_layer_amd import build as hbuild
from hmm_layer_amd import engine

SPECS = pc.all_specs() + pc.refused_cases()
PROFILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "posterior_grad_walk.json")


@pytest.fixture(scope="module")
def lib():
    hbuild.build()
    return engine.lib()


def test_state_range(lib):
    assert lib.hmm_posterior_grad_walk_min_states() == 65 and lib.hmm_posterior_grad_walk_max_states() == 256


def test_validation_order_without_device(lib):
    # shape, q outside 65..256, mode, pointers, then the workspace; nothing here reaches a HIP call
    p = 0x10000                                                                 # never dereferenced
    eps, big = 1e-16, 1 << 40
    k, b, L, q = 2, 3, 17, 71
    f = lib.hmm_posterior_grad_walk
    LOG, PROB, NO_LL = engine.POST_LOG, engine.POST_PROB, engine.POST_LOG_NO_LL
    assert f(None, None, None, k, b, 0, q, eps, 7, None, None, None, None, None, 0, None) == -1
    assert f(None, None, None, k, 0, L, 64, eps, 7, None, None, None, None, None, 0, None) == -1
    assert f(None, None, None, 0, b, L, 257, eps, 7, None, None, None, None, None, 0, None) == -1
    for bad_q in (1, 16, 64, 257, 4096):
        assert f(None, None, None, k, b, L, bad_q, eps, 7, None, None, None, None, None, 0, None) == -2, bad_q
    for bad_mode in (NO_LL, -1, 7):
        assert f(None, None, None, k, b, L, q, eps, bad_mode, None, None, None, None, None, 0, None) == -6, bad_mode
    for mode in (LOG, PROB):
        for hole in range(8):                                                   # A, pi, E, grad_out, dA, dpi, dE, workspace
            a = [p] * 8
            a[hole] = None
            assert f(a[0], a[1], a[2], k, b, L, q, eps, mode, a[3], a[4], a[5], a[6], a[7], 0, None) == -3, hole
        need = lib.hmm_posterior_grad_walk_workspace_bytes(k, b, L, q)
        assert f(p, p, p, k, b, L, q, eps, mode, p, p, p, p, p, need - 1, None) == -4
        assert f(p, p, p, k, b, L, q, eps, mode, p, p, p, p, p + 1, big, None) == -4
    r = lib.hmm_posterior_grad_walk_refused
    assert r(k, b, 0, q, p, big) == -1 and r(k, b, L, 64, p, big) == -2 and r(k, b, L, q, None, big) == -3
    assert r(k, b, L, q, p, need - 1) == -4


def test_workspace_queries(lib):
    query = lib.hmm_posterior_grad_walk_workspace_bytes
    up = lambda n: (n + 255) // 256 * 256                                       # noqa: E731
    for k, b, L, q in ((1, 1, 1, 65), (2, 3, 17, 71), (1, 5, 333, 128), (1, 2, 300, 129), (2, 3, 530, 256),
                      (1, 1024, 1000, 253)):
        w, w1 = query(k, b, L, q), query(k, b, 1, q)
        assert w > 0 and w % 256 == 0, (k, b, L, q)
        # what grows with L: exactly two (k,b,L,q) float arrays, each rounded up to 256 bytes (dE is finished in place)
        assert w - w1 == 2 * (up(4 * k * b * L * q) - up(4 * k * b * q)), (k, b, L, q)
        assert w1 >= 2 * 4 * k * b * 10 * 64 * ((q + 63) // 64)                 # the sequences' accumulators, twice
        assert w < lib.hmm_posterior_grad_large_workspace_bytes(k, b, L, q)
    for q in (1, 16, 64, 257, 1027):
        assert query(2, 3, 17, q) == 0, q
    assert query(0, 3, 17, 71) == 0 and query(2, 0, 17, 71) == 0 and query(2, 3, 0, 71) == 0


def test_pays_is_zero_outside_the_range_and_follows_the_measurements(lib):
    for dims in ((1, 32, 10000, 64), (1, 32, 10000, 257), (0, 32, 10000, 71), (1, 32, 0, 71), (1, 0, 10, 127)):
        assert lib.hmm_posterior_grad_walk_pays(*dims) == 0, dims
    with open(PROFILE) as fh:
        prof = json.load(fh)
    assert prof["margin"] == 1.25
    assert {(q, b) for q in prof["pays"] for b in prof["pays"][q]} == {(str(q), str(b)) for q in pc.GENE_Q for b in (1, 32, 1024)}
    most = 0
    for q, cells in prof["pays"].items():
        for b, cell in cells.items():
            assert cell["pays"] == int(cell["grad_large_over_walk"] >= prof["margin"])
            assert lib.hmm_posterior_grad_walk_pays(1, int(b), prof["L"], int(q)) == cell["pays"], (q, b)
            most = max(most, int(b))
    for q in (65, 71, 128, 129, 256):                                           # more sequences were not measured
        for k, b in ((1, most + 1), (2, most // 2 + 1), (1, 4 * most)):
            assert lib.hmm_posterior_grad_walk_pays(k, b, 10000, q) == 0, (k, b, q)


def test_symbols_are_typed(lib):
    assert set(engine.POSTERIOR_GRAD_WALK_SIGNATURES) == {
        "hmm_posterior_grad_walk_min_states", "hmm_posterior_grad_walk_max_states",
        "hmm_posterior_grad_walk_workspace_bytes", "hmm_posterior_grad_walk_pays", "hmm_posterior_grad_walk_refused",
        "hmm_posterior_grad_walk"}
    for name, (restype, argtypes) in engine.POSTERIOR_GRAD_WALK_SIGNATURES.items():
        assert name not in engine._SIGNATURES and name not in engine.LOGLIK_GRAD_WALK_SIGNATURES
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes)
    assert engine.POSTGRAD_WALK_TAG not in (engine.GRAD_WALK_TAG, engine.WALK_TAG, engine.DECODE_TAG)


def test_wrappers_refuse(lib):
    for q in (16, 64, 257, 1027):
        E = torch.rand(1, 2, 5, q)
        with pytest.raises(ValueError, match="65..256"):
            engine.posterior_grad_walk(torch.eye(q)[None], torch.ones(q) / q, E, torch.ones_like(E))
    A, pi, E = torch.eye(71)[None], torch.ones(71) / 71, torch.rand(1, 2, 5, 71)
    for mode in (engine.POST_LOG_NO_LL, 7):
        with pytest.raises(ValueError, match="POST_PROB or POST_LOG"):          # before the device is asked for
            engine.posterior_grad_walk(A, pi, E, torch.ones_like(E), mode=mode)
    with pytest.raises(engine.EngineError, match="HIP device"):                 # in range: there is no CPU path
        engine.posterior_grad_walk(A, pi, E, torch.ones_like(E))


def test_autograd_posterior_support_only(lib, monkeypatch):
    A, pi, E = torch.eye(71)[None], torch.ones(71) / 71, torch.rand(1, 2, 5, 71)
    for bad in ("yes", 1.5, None, "True"):
        with pytest.raises(ValueError, match="support_only"):
            autograd.posterior(A, pi, E, support_only=bad)
    seen = []
    monkeypatch.setattr(autograd.SupportPosterior, "apply", lambda *a: seen.append("support") or "S")
    monkeypatch.setattr(autograd.Posterior, "apply", lambda *a: seen.append("default") or "D")
    assert autograd.posterior(A, pi, E, support_only="always") == "S"           # does not ask the predicate
    for pays, want in ((1, "S"), (0, "D")):
        monkeypatch.setattr(lib, "hmm_posterior_grad_walk_pays", lambda *dims, _v=pays: _v)
        assert autograd.posterior(A, pi, E, support_only=True) == want
    assert autograd.posterior(A, pi, E) == "D" and autograd.posterior(A, pi, E, support_only=False) == "D"
    # outside 65..256 states the argument is ignored
    A7, pi7 = lc.gene7()
    E7 = torch.rand(1, 2, 9, 7)
    monkeypatch.setattr(lib, "hmm_posterior_grad_walk_pays", lambda *dims: 1)
    for support in ("always", True, False):
        assert autograd.posterior(torch.tensor(A7[None]), torch.tensor(pi7[None]), E7, support_only=support) == "D"
    assert seen.count("support") == 2


@pytest.mark.parametrize("support_grad", [True, False])
def test_the_layer_passes_the_transitioners_flag(monkeypatch, support_grad):
    from hmm_layer_amd import MsaHMMLayer as layer_mod
    from hmm_layer_amd.MsaHmmCell import HmmCell
    from hmm_layer_amd.gene_pred_hmm_emitter import GenePredHMMEmitter
    from hmm_layer_amd.gene_pred_hmm_transitioner import GenePredMultiHMMTransitioner
    from test_loglik_grad_large_gpu import CODONS
    b, L = 2, 12
    g = torch.Generator().manual_seed(13)
    cls = torch.softmax(2 * torch.randn((1, b, L, 15), generator=g), -1)
    nuc = torch.nn.functional.one_hot(torch.randint(0, 4, (1, b, L), generator=g), 5).float()
    x = torch.cat([cls, nuc], -1)
    em = GenePredHMMEmitter(**CODONS, num_copies=5)
    em.build((1, b, L, 15))
    tr = GenePredMultiHMMTransitioner(k=5, initial_exon_len=200, initial_intron_len=4500, initial_ir_len=10000,
                                      support_grad=support_grad)
    cell = HmmCell([71], 15, em, tr)
    layer = layer_mod.MsaHmmLayer(cell, use_prior=False)
    layer.build(x.shape)
    seen = []

    def fake_posterior(A, pi, E, mode=engine.POST_LOG, eps=engine.EPS, support_only=False):
        seen.append((int(mode), support_only))
        return E

    monkeypatch.setattr(layer_mod.autograd, "posterior", fake_posterior)
    monkeypatch.setattr(layer_mod.autograd, "loglik", lambda A, pi, E, **kw: E.sum((2, 3)))
    monkeypatch.setattr(layer_mod, "_graph_inputs",
                        lambda inputs, cell, end_hints, training, what=None: (None, None, torch.ones(1, b, L, 71)))
    monkeypatch.setattr(layer_mod, "_wants_grad", lambda inputs, cell: True)
    layer.state_posterior_log_probs(x, training=True)
    layer.state_posterior_log_probs(x, training=True, no_loglik=True)
    layer.state_posterior_probs(x, training=True)
    assert seen == [(engine.POST_LOG, support_grad), (engine.POST_LOG_NO_LL, support_grad),
                    (engine.POST_PROB, support_grad)]


@pytest.mark.parametrize("spec", SPECS, ids=pc.spec_id)
def test_case_can_carry_the_gpu_comparison(spec):
    c = pc.build(spec)
    k, b, L, q = c["E"].shape
    assert (k, q, b, L) == (len(spec.models), spec.q, spec.b, spec.L) and c["G"].shape == c["E"].shape
    assert all(c[n].dtype == np.float32 for n in ("A", "pi", "E", "G")) and c["A"].shape == (k, q, q)
    assert pc.Q_MIN <= q <= pc.Q_MAX and k * b <= 130 and L <= 300                # every GPU case is small
    if spec.G == "label":
        assert set(np.unique(c["G"])) <= {-1.0, 0.0} and 0.02 < -c["G"].mean() < 0.1
    if k == 2:
        assert not np.array_equal(c["A"][0], c["A"][1])
    assert pc.violations(spec) == []
    for m, ref in enumerate(pc.reference(spec)):
        A = c["A"][m]
        deg = np.maximum((A != 0).sum(0), (A != 0).sum(1))
        if ref is None:
            assert spec.models[m] == pc.REFUSED and (deg > 8).sum() == 3         # outside the sparse rule
            continue
        copies = (q - 1) // 14
        assert (deg > 8).sum() == {"gene": int(copies + 1 > 8), "deg0": 0, "deg1": 1, "deg2": 2}[spec.models[m]]
        assert set(ref["limit"]) == set(pc.FINE_NORMS)
        for n in pc.FINE_NORMS:
            assert ref["small"][n] <= 0.05 and 4 * ref["e32"][n] <= 1e-3, (m, n, ref["small"][n], ref["e32"][n])
            assert ref["limit"][n] == max(3e-4, 4 * ref["e32"][n])
        assert np.all(ref["want"][0][A == 0] == 0.0)                             # the reference on the support of A
        if L == 1:
            assert np.all(ref["want"][0] == 0.0)
        clampedE = c["E"][m] <= spec.eps
        assert np.all(ref["want"][2][clampedE] == 0.0) and np.all(ref["want"][1][c["pi"][m] <= spec.eps] == 0.0)
        if spec.emis == "mid" and spec.eps > pc.EPS:                            # clamped by the caller's eps alone
            assert (clampedE & (c["E"][m] > pc.EPS)).mean() > 0.1
        if spec.models[m] == "deg2":
            assert (c["pi"][m] <= spec.eps).sum() == 2


def test_the_sweep_covers_what_it_is_for():
    specs = pc.all_specs()
    assert len(specs) == 106 and len({pc.spec_id(s) for s in specs}) == len(specs)
    assert set(pc.SEEDS) <= {pc.spec_id(s) for s in specs + pc.refused_cases()}             # no stale entry
    modes = {False, True}
    assert {(s.q, s.L, s.emis, s.G, s.log) for s in pc.gene_sweep()} == \
        {(q, L, e, G, log) for q in (71, 127, 253) for L, e, G in ((120, "holes", "dense"), (41, "rare", "label"),
                                                                   (41, "dead", "dense")) for log in modes}
    for s in pc.gene_sweep():
        if s.emis in ("holes", "rare"):
            assert {"forward", "backward"} <= pc.engages(s)[0]
    emis, Gs = ("holes", "rare", "mid"), ("dense", "label")
    assert {(s.models[0], s.q, s.emis, s.G, s.log) for s in pc.state_sweep()} == \
        {(kind, q, emis[(n + i) % 3], Gs[(n + i) % 2], log) for n, q in enumerate((65, 96, 128, 129, 192, 193, 256))
         for i, kind in enumerate(("deg0", "deg1", "deg2")) for log in modes}
    assert all(s.L == 17 and s.b == 3 for s in pc.state_sweep())
    assert {(s.q, s.models, s.L, s.log) for s in pc.length_sweep()} == \
        {(q, ms, L, log) for q, ms in ((71, ("gene", "deg1")), (193, ("deg2", "deg0")))
         for L in (1, 2, 3, 7, 8, 9, 17, 300) for log in modes}
    assert {(s.b, s.L, s.models, s.log) for s in pc.batch_sweep()} == \
        {(b, 24, ("gene", "deg2") if b < 130 else ("gene",), log) for b in (1, 3, 65, 130) for log in modes}
    assert {(s.models, s.q, s.b, s.L, s.emis) for s in pc.eps_cases()} == \
        {(("gene", "deg1"), 71, 4, 12, "mid"), (("deg1",), 253, 4, 12, "mid"), (("gene",), 71, 3, 9, "dead")}
    assert all(s.eps == 1e-6 for s in pc.eps_cases()) and "forward" in pc.engages(pc.eps_cases()[-1])[0]
    assert all(s.models == ("deg3", "deg1") and s.q == 96 and s.L == 17 for s in pc.refused_cases())


def test_build_is_deterministic_and_read_only():
    s = pc.state_sweep()[0]
    a = pc.build(s)
    pc._build.cache_clear()
    b = pc.build(s)
    assert a is not b and all(np.array_equal(a[n], b[n]) for n in a)
    assert pc.build(s._replace(log=not s.log)) is b                             # both modes share their arrays
    with pytest.raises(ValueError):
        a["E"][0, 0, 0, 0] = 1.0
