"""Keeps tests/postgrad_mid_cases.py honest without a GPU: from the fp64 oracle alone, every case of
tests/test_postgrad_mid_gpu.py has finite gradients, few enough columns / rows under the small-scale rule, an fp32 twin
far inside the limit under every norm, and its clamps engaged in the fp64 recursion."""
import numpy as np
import pytest

import postgrad_mid_cases as pc


@pytest.mark.parametrize("spec", pc.all_specs(), ids=pc.spec_id)
def test_case_can_carry_the_gpu_comparison(spec):
    c = pc.build(spec)
    k, b, L, q = c["E"].shape
    assert (k, q, b, L) == (len(spec.models), spec.q, spec.b, spec.L)
    assert all(c[n].dtype == np.float32 for n in ("A", "pi", "E", "G"))
    assert b * L * q <= max(130 * 24 * 43, 3 * 203 * 64)
    if k == 2:
        assert not np.array_equal(c["A"][0], c["A"][1])                 # the models of a call differ
    for m, ref in enumerate(pc.reference(spec)):
        assert all(np.isfinite(x).all() for x in ref["want"]), m
        assert np.abs(c["A"][m].astype(np.float64).sum(-1) - 1).max() < 1e-5
        for n in pc.FINE_NORMS:
            assert ref["small"][n] <= 0.05, (m, n, ref["small"][n])
            assert pc.FINE_FACTOR * ref["e32"][n] < pc.FINE_CAP, (m, n, ref["e32"][n])
            assert ref["limit"][n] == max(pc.FINE_FLOOR, pc.FINE_FACTOR * ref["e32"][n])
        assert ref["e32"]["tensor"] <= pc.TENSOR_REL / pc.FINE_FACTOR
        gam, count = pc.forward_backward64(c["A"][m], c["pi"][m], c["E"][m])
        assert np.abs(gam.sum(-1) - 1).max() <= 1e-12
        for clamp in pc.engages(spec)[m]:
            assert count[clamp] >= 1, (m, clamp, count)
        if spec.G == "label":                                           # one label per position, on its most probable state
            assert np.array_equal(c["G"][m], -(gam == gam.max(-1, keepdims=True)).astype(np.float32))
            assert np.all(c["G"][m].sum(-1) == -1.0)
            if spec.log:                                                # nothing of the weight on a negligible state
                assert gam[c["G"][m] < 0].min() > 1.0 / (2 * q)


def test_the_sweep_covers_what_it_is_for():
    specs = pc.all_specs()
    assert len({pc.spec_id(s) for s in specs}) == len(specs)
    sweep = [s for s in specs if (s.b, s.L) == (pc.SWEEP_B, pc.SWEEP_L)]
    assert pc.SWEEP_L % 8 == 3 and pc.SWEEP_L // 8 == 25                # MQ_PF = 8: whole blocks and a tail
    for log in pc.MODES:
        qs = {s.q for s in sweep if s.log == log}
        assert qs == set(pc.STATE_Q) | set(pc.GENE_Q)
        for lo, hi in ((17, 32), (33, 48), (49, 64)):                   # each QB: both ends, and lanes idle inside the block
            assert {lo, hi} <= qs and any(lo < q < hi for q in qs)
        for q in pc.GENE_Q:
            assert {(s.emis, s.G) for s in sweep if s.log == log and s.q == q} == \
                {("holes", "dense"), ("rare", "label"), ("dead", "label")}
        kinds = [s.models[0] for s in sweep if s.log == log and s.q in pc.STATE_Q]
        assert kinds.count("dense") >= 4 and kinds.count("sparse") >= 4
        assert {(s.q, s.L) for s in pc.length_sweep() if s.log == log} == {(q, L) for q in (33, 43, 57) for L in pc.LENGTHS}
        assert {s.b for s in pc.batch_sweep() if s.log == log} == {1, 64, 65, 130}
        assert {(s.q, s.models[0]) for s in pc.clamp_cases() if s.log == log} == \
            {(40, "fclamp"), (40, "bclamp"), (60, "fclamp"), (60, "bclamp")}
    assert all(len(s.models) == 2 for s in pc.length_sweep() + pc.batch_sweep())
    assert all(s.G == "label" for s in specs if s.log and s.emis in ("rare", "dead"))
    assert set(pc.SEEDS) <= {pc.spec_id(s) for s in specs}                  # no stale entry in the table of replaced seeds


def test_build_is_deterministic_and_read_only():
    s = pc.state_sweep()[0]
    a = pc.build(s)
    pc._build.cache_clear()
    b = pc.build(s)
    assert a is not b and all(np.array_equal(a[n], b[n]) for n in a)
    with pytest.raises(ValueError):
        a["E"][0, 0, 0, 0] = 1.0
    with pytest.raises(ValueError):
        pc.reference(s)[0]["want"][2][0, 0, 0] = 1.0


def test_norms_see_a_wrong_column_a_wrong_sequence_and_a_wrong_row():
    """What the tensor norm lets pass: an error of 1e-3 of ONE column's, sequence's or row's own scale, where that scale
    is 1e-3 of the tensor's."""
    rng = np.random.default_rng(0)
    q, b, L = 33, 3, 20
    A = np.asarray(pc.rand_model(rng, q, sparse=True)[0])
    wA, wpi, wE = rng.standard_normal((q, q)), rng.standard_normal(q), rng.standard_normal((b, L, q))
    wE[..., 5] *= 1e-3
    wE[1] *= 1e-3
    i = int(np.argmax((A > 0).sum(-1)))
    wA[i] *= 1e-3
    clean, _ = pc.errors((wA, wpi, wE), (wA, wpi, wE), A)
    assert all(v <= 0 for v in clean.values())
    for norm, where in (("dE/col", (2, (0, 3, 5))), ("dE/seq", (2, (1, 7, 2))), ("dA/row", (0, (i, int(np.argmax(A[i] > 0)))))):
        got = [wA.copy(), wpi.copy(), wE.copy()]
        t, idx = where
        got[t][idx] += 1e-3 * np.abs((wA, wpi, wE)[t][idx[0]] if norm != "dE/col" else wE[..., 5]).max()
        e, _ = pc.errors(got, (wA, wpi, wE), A)
        assert e["tensor"] < pc.TENSOR_REL and e[norm] > pc.FINE_FLOOR, (norm, e)
        assert all(e[n] <= pc.FINE_FLOOR for n in pc.FINE_NORMS if n != norm), (norm, e)
