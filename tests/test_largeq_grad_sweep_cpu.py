"""Keeps tests/largeq_grad_cases.py honest without a GPU: from the fp64 oracles alone, every case of
tests/test_largeq_grad_sweep_gpu.py has finite gradients, few enough rows / columns / sequences under the exclusion
rule, an fp32 twin far inside the cap under every finer norm, and its clamps and holes engaged in the fp64 recursion;
the case lists contain the boundary values they are for; and the three tile-width shapes select 64, 80 and 96 columns
under the restated lq_tile_width."""
import numpy as np
import pytest

import largeq_grad_cases as lg

SPECS = lg.all_specs() + [lg.composition_case()]


@pytest.mark.parametrize("spec", SPECS, ids=lg.spec_id)
def test_case_can_carry_the_gpu_comparison(spec):
    c = lg.build(spec)
    k, b, L, q = c["E"].shape
    assert (k, q, b, L) == (len(spec.models), spec.q, spec.b, spec.L)
    assert all(c[n].dtype == np.float32 for n in ("A", "pi", "E")) and c["A"].shape == (k, q, q) and c["pi"].shape == (k, q)
    assert spec.route in lg.ROUTES and (q <= lg.WALK_MAX or spec.route in ("lgemm", "pgemm"))
    if lg.kind(spec) == "l":
        assert c["G"] is None and (c["w"] is None) == (spec.w == "none")
        if c["w"] is not None:
            assert c["w"].dtype == np.float32 and c["w"].shape == (k, b)
            live = np.abs(c["w"][c["w"] != 0])
            assert live.min() >= 1e-3 * (1 - 1e-6) and live.max() <= 1e3 * (1 + 1e-6)
            assert (c["w"] == 0).sum() == (3 * k if spec.w == "zeros" else 0)
    else:
        assert c["w"] is None and c["G"].dtype == np.float32 and c["G"].shape == c["E"].shape
        if spec.G == "label":
            assert set(np.unique(c["G"])) == {-1.0, 0.0}
    assert b * L * q <= 3328 * 2 * 344 and (q <= 130 or L <= 64)
    if k == 2:
        assert not np.array_equal(c["A"][0], c["A"][1])                 # the models of a call differ
    assert lg.violations(spec) == []
    floor = 2e-4 if lg.kind(spec) == "l" else 3e-4
    for m, ref in enumerate(lg.reference(spec)):
        rows = c["A"][m].astype(np.float64).sum(-1)
        assert np.all(np.abs(rows - 1) < 1e-5)
        assert set(ref["limit"]) == set(lg.FINE_NORMS)
        for n in lg.FINE_NORMS:
            assert ref["small"][n] <= 0.05 and 4 * ref["e32"][n] <= 1e-3, (m, n, ref["small"][n], ref["e32"][n])
            assert ref["limit"][n] == max(floor, 4 * ref["e32"][n])
        if lg.kind(spec) == "l":
            assert np.isfinite(ref["dA_unmasked"]).all()
        if L == 1:
            assert np.all(ref["want"][0] == 0.0)
        if spec.w == "zeros":
            assert np.all(ref["want"][2][c["w"][m] == 0] == 0.0)
        clampedE = c["E"][m] <= spec.eps
        assert np.all(ref["want"][2][clampedE] == 0.0) and np.all(ref["want"][1][c["pi"][m] <= spec.eps] == 0.0)
        if spec.emis == "mid":                                          # clamped by the caller's eps alone
            assert (clampedE & (c["E"][m] > lg.EPS)).mean() > 0.1
        if spec.emis == "blank0":
            assert np.all(c["E"][m, lg.heaviest(c, m), 0] == 0.0) and (c["E"][m, :, 0] == 0.0).all(-1).sum() == 1
        if any(n in spec.models for n in ("tinypi", "deadin")) and spec.models[m] in ("tinypi", "deadin"):
            assert (c["pi"][m] <= spec.eps).sum() == 2


def test_the_composition_case_shows_the_lost_first_row():
    """POST_LOG_NO_LL adds the log-likelihood gradient with weights sum of G: the blank first row's sequence carries
    far more of dpi than the 3e-4 tensor norm lets pass."""
    spec = lg.composition_case()
    assert (spec.route, spec.q, spec.emis, spec.log) == ("pwalk", 80, "blank0", True) and spec.q > 64
    want = lg.composition_reference(spec)
    share = lg.blank0_share(spec, lg.build(spec), 0)
    assert share > 100 * 3e-4 * np.abs(want[1]).max(), (share, np.abs(want[1]).max())


def test_the_sweep_covers_what_it_is_for():
    specs = lg.all_specs()
    assert len({lg.spec_id(s) for s in specs}) == len(specs)
    assert set(lg.SEEDS) <= {lg.spec_id(s) for s in specs + [lg.composition_case()]}    # no stale entry
    modes = lambda ss: {s.log for s in ss}                              # noqa: E731
    walk = lg.walk_state_sweep()
    for route in ("lwalk", "pwalk"):
        ws = [s for s in walk if s.route == route]
        assert all((s.b, s.L) == (3, 41) and s.w in ("wide", "") for s in ws)
        assert {s.q for s in ws if s.models != ("gene",)} == {65, 66, 67, 68, 69, 96, 127, 128, 1, 2, 3, 4, 5, 33, 63, 64}
        assert {s.models for s in ws} == {("dense",), ("sparse",), ("gene",)}
        assert {s.emis for s in ws if s.models != ("gene",)} == {"holes", "rare"}
        assert {(s.q, s.emis) for s in ws if s.models == ("gene",)} == {(71, "holes"), (71, "rare"), (71, "dead")}
    assert modes(s for s in walk if s.route == "pwalk") == {False, True}
    gemm = lg.gemm_state_sweep()
    for route in ("lgemm", "pgemm"):
        gs = [s for s in gemm if s.route == route]
        assert {s.q for s in gs} == {1, 15, 16, 17, 31, 32, 33, 64, 65, 95, 96, 97, 127, 128, 129, 159, 160, 161, 191, 192,
                                     193, 255, 256, 257}
        assert all((s.b, s.L) == (3, 9) for s in gs) and {s.models for s in gs} == {("dense",), ("sparse",)}
    assert modes(s for s in gemm if s.route == "pgemm") == {False, True}
    assert {(s.route, s.q, s.L) for s in lg.length_sweep()} == \
        {(r, 90, L) for r in lg.ROUTES for L in (1, 2, 3, 4, 5)} \
        | {(r, 130, L) for r in ("lgemm", "pgemm") for L in (1, 2, 3, 4, 5)}
    assert {(s.route, s.q, s.b, s.L) for s in lg.batch_sweep()} == \
        {(r, q, b, 6) for q, rs in ((71, lg.ROUTES), (140, ("lgemm", "pgemm"))) for r in rs
         for b in (1, 4, 5, 15, 16, 17, 63, 64, 65, 130)}
    assert {s.models for s in lg.batch_sweep() if s.q == 71} == {("gene", "sparse")}
    assert {s.models for s in lg.batch_sweep() if s.q == 140} == {("dense", "sparse")}
    assert all(len(s.models) == 2 and s.models[0] != s.models[1] for s in lg.length_sweep() + lg.batch_sweep())
    for ss in (lg.length_sweep(), lg.batch_sweep()):
        assert modes(s for s in ss if s.route[0] == "p") == {False, True}
    assert {(s.route, s.b, s.q, s.L) for s in lg.tile_cases()} == \
        {(r, b, q, 2) for r in ("lgemm", "pgemm") for b, q in ((192, 1027), (3328, 261), (3328, 344))}
    wl = [s for s in lg.weight_cases() if s.route[0] == "l"]
    for route, q in (("lwalk", 90), ("lgemm", 90), ("lgemm", 200)):
        ws = [s for s in wl if (s.route, s.q) == (route, q)]
        assert {s.w for s in ws} == {"zeros", "none", "wide"} and {"blank0", "holes"} == {s.emis for s in ws}
        assert any("tinypi" in s.models for s in ws) and any("deadin" in s.models for s in ws)
        assert any(s.w == "zeros" and s.b > 64 for s in ws)             # k_mq_grad_pi beyond one stride with zero weights
    wp = [s for s in lg.weight_cases() if s.route[0] == "p"]
    assert {(s.route, s.emis == "blank0", "tinypi" in s.models, s.G, s.log) for s in wp} == \
        {(r, x, not x, G, log) for r in ("pwalk", "pgemm") for x in (True, False) for G in ("dense", "label")
         for log in (False, True)}
    assert {(s.route, s.eps, s.emis) for s in lg.eps_cases()} == {(r, 1e-6, "mid") for r in lg.ROUTES}
    cl = lg.clamp_cases()
    assert all(s.L == 60 and (s.w == "wide" or s.G == "dense") for s in cl)
    assert {(s.route, s.q, s.models[0]) for s in cl} == \
        {(r, 70, "fclamp") for r in lg.ROUTES} | {(r, 150, "fclamp") for r in ("lgemm", "pgemm")} \
        | {(r, 70, "bclamp") for r in ("pwalk", "pgemm")} | {("pgemm", 150, "bclamp")}
    assert modes(s for s in cl if s.route[0] == "p") == {False, True}
    for q in (128, 129):                                                # the default route on either side of the switch
        assert any(s.q == q for s in walk + gemm)


def test_tile_width_shapes():
    """The rule of lq_tile_width restated in Python (tests/largeq_sweep.py); the GPU file asserts the same through the
    engine.  q is no multiple of the width for 80 and 96; the 64-column shape has a batch of three 64-row tiles."""
    assert {cols for _, _, cols in lg.TILE_SHAPES} == {64, 80, 96}
    for b, q, cols in lg.TILE_SHAPES:
        assert lg.tile_cols(b, q) == cols and q % cols != 0
    assert all(lg.tile_cols(3328, q) == 80 for q in range(257, 289)) and lg.tile_cols(192, 1027) == 64 and 192 > 64
    for s in lg.gemm_state_sweep() + lg.length_sweep() + lg.batch_sweep():
        assert lg.tile_cols(s.b, s.q) == 64                             # every small shape: 64 columns
    assert lg.tile_cols(1024, 1027) == 80                               # test_config5_shape_1027_states


def test_build_is_deterministic_and_read_only():
    for s in (lg.walk_state_sweep()[0], lg.weight_cases()[-1], lg.eps_cases()[0]):
        a = lg.build(s)
        lg._build.cache_clear()
        b = lg.build(s)
        assert a is not b and all(np.array_equal(a[n], b[n]) if a[n] is not None else b[n] is None for n in a)
    with pytest.raises(ValueError):
        a["E"][0, 0, 0, 0] = 1.0
    with pytest.raises(ValueError):
        lg.reference(s)[0]["want"][2][0, 0, 0] = 1.0
    # the two evaluations of an entry point and the two modes share their arrays
    x = [t for t in lg.length_sweep() if (t.q, t.L) == (90, 3)]
    assert len({id(lg.build(t)) for t in x}) == 2 and len(x) == 6
    one = [t for t in lg.all_specs() if lg.spec_id(t) == lg.spec_id(x[0])]
    assert one == [x[0]]                                                # a case can be rerun alone from its id


def test_norms_see_a_wrong_row_a_wrong_sequence_and_a_wrong_column():
    """What the tensor norm of the posterior gradients lets pass (the log-likelihood side: the test of this name in
    tests/test_loglik_grad_sweep_cpu.py): a dA row, a sequence or a state column whose scale is 1e-4 of the tensor's."""
    rng = np.random.default_rng(0)
    q, b, L = 70, 3, 6
    A = np.asarray(lg.lc.rand_model(rng, q, sparse=True)[0])
    spec = lg.length_sweep()[-1]
    assert lg.kind(spec) == "p"
    wA, wpi, wE = rng.standard_normal((q, q)), rng.standard_normal(q), rng.standard_normal((b, L, q))
    wE[..., 5] *= 1e-4
    wE[1] *= 1e-4
    wA[7] *= 1e-4
    ref = dict(want=(wA, wpi, wE))
    clean, _ = lg.errors(spec, (wA, wpi, wE), ref, A)
    assert all(v <= 0 for v in clean.values())
    for norm in lg.FINE_NORMS:
        got = [wA.copy(), wpi.copy(), wE.copy()]
        if norm == "dA/row":
            got[0][7] *= 2
        elif norm == "dE/seq":
            got[2][1] *= 1.03
        else:
            got[2][..., 5] *= 1.03
        e, _ = lg.errors(spec, got, ref, A)
        assert e["tensor"] <= 3e-4 and e[norm] > 0.02, (norm, e)
        assert all(e[n] <= 3e-4 for n in lg.FINE_NORMS if n != norm), (norm, e)
