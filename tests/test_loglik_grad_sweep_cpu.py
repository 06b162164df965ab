"""Keeps tests/loglik_grad_cases.py honest without a GPU: from the fp64 oracle alone, every case of
tests/test_loglik_grad_sweep_gpu.py has finite gradients, few enough rows / columns / sequences under the exclusion
rules, an fp32 twin far inside the cap under every finer norm, and its clamps and holes engaged in the fp64 recursion;
and the case lists contain the boundary values they are for."""
import numpy as np
import pytest

import loglik_grad_cases as lc


@pytest.mark.parametrize("spec", lc.all_specs(), ids=lc.spec_id)
def test_case_can_carry_the_gpu_comparison(spec):
    c = lc.build(spec)
    k, b, L, q = c["E"].shape
    assert (k, q, b, L) == (len(spec.models), spec.q, spec.b, spec.L)
    assert all(c[n].dtype == np.float32 for n in ("A", "pi", "E")) and c["A"].shape == (k, q, q) and c["pi"].shape == (k, q)
    assert (c["w"] is None) == (spec.w == "none")
    if c["w"] is not None:
        assert c["w"].dtype == np.float32 and c["w"].shape == (k, b)
        live = np.abs(c["w"][c["w"] != 0])
        assert live.min() >= 1e-3 * (1 - 1e-6) and live.max() <= 1e3 * (1 + 1e-6)
        assert (c["w"] == 0).sum() == (3 * k if spec.w == "zeros" else 0)
    assert b * L * q <= 130 * 24 * 43
    if k == 2:
        assert not np.array_equal(c["A"][0], c["A"][1])                 # the models of a call differ
    assert spec.route in lc.ROUTES and (q <= 16) == (spec.route == "scan16")
    for m, ref in enumerate(lc.reference(spec)):
        assert all(np.isfinite(x).all() for x in ref["want"]) and np.isfinite(ref["dA_unmasked"]).all(), m
        rows = c["A"][m].astype(np.float64).sum(-1)
        assert np.all((np.abs(rows - 1) < 1e-5) | ((rows == 0) & (spec.models[m] == "shipped")))
        assert set(ref["limit"]) == set(lc.fine_norms(spec.route))
        for n in lc.fine_norms(spec.route):
            assert ref["small"][n] <= lc.SMALL_CAP, (m, n, ref["small"][n])
            assert lc.FINE_FACTOR * ref["e32"][n] <= lc.FINE_CAP, (m, n, ref["e32"][n])
            assert ref["limit"][n] == max(lc.FINE_FLOOR, lc.FINE_FACTOR * ref["e32"][n])
        _, count = lc.forward_backward64(c["A"][m], c["pi"][m], c["E"][m])
        for clamp in lc.engages(spec)[m]:
            assert count[clamp] >= 1, (m, clamp, count)
        if L == 1:
            assert np.all(ref["want"][0] == 0.0)
        if c["w"] is not None:
            assert np.all(ref["want"][2][c["w"][m] == 0] == 0.0)
        assert np.all(ref["want"][2][c["E"][m] <= lc.EPS] == 0.0) and np.all(ref["want"][1][c["pi"][m] <= lc.EPS] == 0.0)
    if spec.emis == "blank0":                                           # dpi's share of the blank first row is not negligible
        for m, ref in enumerate(lc.reference(spec)):
            s = int(np.abs(c["w"][m]).argmax())
            assert np.all(c["E"][m, s, 0] == 0.0)
            alone = lc.textbook.loglik_grad(c["A"][m], c["pi"][m], c["E"][m, s:s + 1], c["w"][m, s:s + 1])[1]
            assert np.abs(alone).max() > 0.5 * np.abs(ref["want"][1]).max()
    if spec.emis == "stretch":
        t0, s, j = L // 2, lc.STRETCH_SEQ, lc.STRETCH_STATE
        only = np.zeros(q, bool)
        only[j] = True
        assert np.all((c["E"][0, s, t0:t0 + lc.STRETCH_LEN] > 0) == only)
        assert (c["A"][0, j] > 0).sum() == 1 and c["A"][0, j, j] == 0   # left after one step
        assert (c["E"][0, [x for x in range(b) if x != s]] > 0).all()


def test_the_sweep_covers_what_it_is_for():
    specs = lc.all_specs()
    assert len({lc.spec_id(s) for s in specs}) == len(specs)
    assert lc.SWEEP_L % 8 == 3 and lc.SWEEP_L // 8 == 25                # MQ_PF = 8: whole blocks and a tail
    wave = [s for s in lc.wave_state_sweep()]
    assert all((s.route, s.b, s.L, s.w) == ("wave", 3, 203, "wide") for s in wave)
    for kind in ("dense", "sparse"):
        assert {s.q for s in wave if s.models == (kind,)} == {17, 31, 32, 33, 47, 48, 49, 63, 64}
        assert {s.emis for s in wave if s.models == (kind,)} == {"holes", "rare"}
    for q in (29, 43, 57):
        assert {s.emis for s in wave if s.models == ("gene",) and s.q == q} == {"holes", "rare", "dead"}
    scan = lc.scan16_state_sweep()
    assert all((s.route, s.b, s.L, s.w) == ("scan16", 3, 203, "wide") for s in scan)
    assert {s.q for s in scan if s.models[0] != "gene"} == {1, 2, 3, 4, 5, 8, 9, 12, 13, 15, 16}
    assert {s.q for s in scan if s.models[0] == "gene"} == {7, 15}
    assert {s.emis for s in scan} == {"holes", "rare"}                  # dead: on the wave route only
    assert {(s.route, s.q, s.L) for s in lc.length_sweep()} == \
        {(r, q, L) for r, qs in (("wave", (32, 43, 64)), ("scan16", (6, 15))) for q in qs for L in (1, 2, 7, 8, 9, 15, 16, 17)}
    assert {(s.route, s.q, s.b, s.L) for s in lc.batch_sweep()} == \
        {(r, q, b, 24) for r, q in (("wave", 43), ("scan16", 15)) for b in (63, 64, 65, 130)}
    assert all(len(s.models) == 2 and s.models[0] != s.models[1] for s in lc.length_sweep() + lc.batch_sweep())
    for route in ("wave", "scan16"):
        ws = [s for s in lc.weight_cases() if s.route == route]
        assert {"zeros", "none", "wide"} <= {s.w for s in ws} and any("tinypi" in s.models for s in ws)
        assert any(s.w == "zeros" and s.b > 64 for s in ws)             # k_*grad_pi beyond one stride with zero weights
    assert {(s.route, s.q, s.models) for s in lc.clamp_cases()} == {("wave", 40, ("fclamp",)), ("wave", 60, ("fclamp",))}
    w = lc.window_case()
    assert (w.route, w.models, w.q, w.chunk, w.emis) == ("scan16", ("gene",), 15, 16, "stretch") and w.L >= 4 * w.chunk
    s = lc.shipped_case()
    assert (s.route, s.models, s.chunk) == ("scan16", ("shipped",), 16) and not lc.primitive(s)
    assert {(s.b, s.L, s.chunk) for s in lc.pc29_cases() if s.emis == "holes"} == {(3, 333, 16), (2, 700, 0), (5, 97, 16)}
    assert all((s.route, s.models, s.q, s.w) == ("pc29", ("gene",), 29, "wide") for s in lc.pc29_cases())
    assert {s.route for s in specs if s.emis == "blank0"} == {"wave", "scan16", "pc29"}
    g = lc.gscan_cases()
    assert {(s.models[0] == "gene", s.q) for s in g} == {(False, 17), (False, 32), (False, 33), (False, 49), (False, 64),
                                                         (True, 43), (True, 57)}
    assert all((s.route, s.L, s.chunk) == ("gscan", 203, 16) and lc.primitive(s) for s in g)
    for s in g:                                                         # the wave case's arrays, not a copy
        assert any(lc.build(s) is lc.build(v) for v in wave)
    assert set(lc.SEEDS) <= {lc.spec_id(s) for s in specs}              # no stale entry in the table of replaced seeds


def test_build_is_deterministic_and_read_only():
    for s in (lc.wave_state_sweep()[0], lc.weight_cases()[0], lc.window_case()):
        a = lc.build(s)
        lc._build.cache_clear()
        b = lc.build(s)
        assert a is not b and all(np.array_equal(a[n], b[n]) for n in a)
    with pytest.raises(ValueError):
        a["E"][0, 0, 0, 0] = 1.0
    with pytest.raises(ValueError):
        lc.reference(s)[0]["want"][2][0, 0, 0] = 1.0


def test_norms_see_a_wrong_row_a_wrong_sequence_and_a_wrong_column():
    """What the tensor norms let pass: a row of dA off by a factor of two where its scale is 1e-5 of the tensor's, and
    every dE entry of one sequence (one column) off by 3 % where that sequence's (column's) scale is 1e-4 of the
    tensor's."""
    rng = np.random.default_rng(0)
    q, b, L = 33, 3, 20
    A = np.asarray(lc.rand_model(rng, q, sparse=True)[0])
    wA, wpi, wE, wll = rng.standard_normal((q, q)), rng.standard_normal(q), rng.standard_normal((b, L, q)), rng.standard_normal(b)
    wE[..., 5] *= 1e-4
    wE[1] *= 1e-4
    i = int(np.argmax((A > 0).sum(-1)))
    wA[i] *= 1e-5
    ref = dict(want=(wA, wpi, wE, wll), dA_unmasked=wA, dead=np.zeros(q, bool))
    clean, small = lc.errors((wA, wpi, wE, wll), ref, A, "wave")
    assert all(v == 0 for v in clean.values()) and all(v == 0 for v in small.values())
    for norm in ("dA/row", "dE/seq", "dE/col"):
        got = [wA.copy(), wpi.copy(), wE.copy(), wll.copy()]
        if norm == "dA/row":
            got[0][i] *= 2
        elif norm == "dE/seq":
            got[2][1] *= 1.03
        else:
            got[2][..., 5] *= 1.03
        e, _ = lc.errors(got, ref, A, "wave")
        assert all(e[n] <= 1 for n in lc.TENSOR_NORMS) and e[norm] > 100 * lc.FINE_FLOOR, (norm, e)
        assert all(e[n] <= lc.FINE_FLOOR for n in lc.fine_norms("wave") if n != norm), (norm, e)
    # the scan routes: no dE/col, and the dA row of a state that is dead in the reference is left to the tensor norm
    got = [wA.copy(), wpi, wE, wll]
    got[0][i] *= 2
    dead = np.zeros(q, bool)
    dead[i] = True
    e, small = lc.errors(got, dict(ref, dead=dead), A, "scan16")
    assert "dE/col" not in e and e["dA/row"] == 0 and small["dA/row"] == 1 / q
