"""Keeps tests/largeq_sweep.py honest without a GPU: the draw is deterministic, the committed (N, seed) meets the
coverage conditions, the fp64 reference is well-conditioned on every drawn case, the Python restatement of the GEMM's
tile-width rule gives what tests/test_configs_gpu.py asserts on the device, and the long five-copy case of
tests/test_largeq_sweep_gpu.py is known to reach the fp32 underflow of the parked product before anyone goes to the
GPU."""
import numpy as np

import largeq_sweep as sweep
from largeq_sweep import N_CASES, SEED, long_five_copy_case, lq_tile_width


def shapes():
    return [sweep.draw_shape(sweep.case_rng(SEED, i)) for i in range(N_CASES)]


def test_draw_case_is_deterministic_for_a_seed():
    for i in (0, 3, 11):
        a, b = sweep.draw_case(sweep.case_rng(SEED, i)), sweep.draw_case(sweep.case_rng(SEED, i))
        assert a.keys() == b.keys()
        for key in a:
            assert np.array_equal(a[key], b[key]), (i, key)
        s = sweep.draw_shape(sweep.case_rng(SEED, i))                 # the shape is the first thing a case draws
        assert all(a[key] == s[key] for key in s), i
    a, b = sweep.draw_case(sweep.case_rng(SEED, 0)), sweep.draw_case(sweep.case_rng(SEED + 1, 0))
    assert a["E"].shape != b["E"].shape or not np.array_equal(a["E"], b["E"])


def test_committed_sweep_meets_the_coverage_conditions():
    sh = shapes()
    cv = sweep.coverage(sh)
    qs = {s["q"] for s in sh}
    for triple in sweep.Q_TRIPLES:                                    # 65, 66, 67 and n-1, n, n+1 of every boundary n
        assert all(q in qs for q in triple), (triple, cv["boundary_missing"])
    assert cv["boundary_missing"] == []
    assert cv["residues"] == [0, 1, 2, 3]
    assert cv["slab_full"] >= 1 and cv["slab_tail"] >= 1              # q % 32 == 0 and != 0
    assert all(n >= 2 for n in cv["kinds"].values()), cv["kinds"]
    assert set(cv["kinds"]) == set(sweep.KINDS) and len(sweep.KINDS) == 8
    assert all(n >= 2 for n in cv["zeros"].values()), cv["zeros"]
    assert cv["ragged_multi"] >= 3                                    # k >= 2 with b not a multiple of 64
    assert all(n >= 1 for n in cv["lengths"].values()), cv["lengths"]
    assert cv["long"] >= 1                                            # one of L = 3000 / 3001
    assert cv["eps_large"] >= 1
    assert sweep.covered(cv)
    assert all(s["q"] == 71 for s in sh if s["kind"] == "gene5")
    assert all(65 <= s["q"] <= 600 and s["k"] in sweep.K_POOL and s["b"] in sweep.B_POOL
               and s["L"] in sweep.L_POOL + sweep.L_LONG for s in sh)
    assert all(s["q"] <= 130 and s["b"] <= 4 for s in sh if s["L"] in sweep.L_LONG)


def test_seed_is_the_first_that_covers():
    """How the committed seed was chosen: no seed below it meets the conditions with N_CASES cases."""
    assert sweep.search_seed(N_CASES, range(SEED + 1)) == SEED


def test_degenerate_models_are_rejected_in_the_draw():
    q = 70
    assert not sweep.model_is_usable(np.zeros((q, q), np.float32))            # every row zero
    bad = np.eye(q, dtype=np.float32)
    bad[3, 3] = np.nan
    assert not sweep.model_is_usable(bad)
    assert not sweep.model_is_usable(np.eye(q, dtype=np.float32) * 0.5)       # rows that sum to neither 1 nor 0
    ok = np.eye(q, dtype=np.float32)
    ok[5] = 0
    assert sweep.model_is_usable(ok)


def test_reference_is_well_conditioned_on_every_drawn_case():
    for i in range(N_CASES):
        c = sweep.draw_case(sweep.case_rng(SEED, i))
        k, b, L, q = c["E"].shape
        assert (k, b, L, q) == (c["k"], c["b"], c["L"], c["q"]) and c["A"].shape == (k, q, q) and c["pi"].shape == (k, q)
        assert c["A"].dtype == c["pi"].dtype == c["E"].dtype == np.float32
        if k >= 2 and c["kind"] != "identity":
            assert not np.array_equal(c["A"][0], c["A"][1]), i                 # the models of a call differ
        if k >= 2:
            assert not np.array_equal(c["pi"][0], c["pi"][1]), i
        for m in range(k):
            assert sweep.model_is_usable(c["A"][m]), (i, m)
            o = sweep.oracle(c["A"][m], c["pi"][m], c["E"][m], c["eps"])
            assert np.isfinite(o["g"]).all() and np.isfinite(o["ll"]).all(), (i, m)
            assert np.abs(o["g"].sum(-1) - 1).max() <= 1e-12, (i, m)
            assert not np.isnan(o["la"]).any() and not np.isnan(o["lb"]).any(), (i, m)


def test_tile_width_restatement():
    assert lq_tile_width(1024, 1027) == 5 and lq_tile_width(3328, 344) == 6 and lq_tile_width(192, 1027) == 4
    # the shapes tests/test_largeq_sweep_gpu.py runs: ragged tile map, odd number of tile columns, q % 16 != 0
    for b, q, ntw in ((300, 3375, 5), (321, 3500, 6)):
        mt, nt = -(-b // 64), -(-q // (16 * ntw))
        assert lq_tile_width(b, q) == ntw and mt % 4 != 0 and nt % 2 == 1 and q % 16 != 0 and b % 64 != 0
    assert lq_tile_width(2, 4096) == 4 and -(-4096 // 64) == 64               # the partial-sum row is exactly full


def test_long_five_copy_case_reaches_the_fp32_underflow():
    for L in (4000, 4001):
        c = long_five_copy_case(L)
        assert c["q"] == 71 and abs(c["zero"] - 0.47) < 0.01
        o = sweep.oracle(c["A"][0], c["pi"][0], c["E"][0], c["eps"])
        assert np.isfinite(o["g"]).all() and np.abs(o["g"].sum(-1) - 1).max() <= 1e-12
        zeros, rows = sweep.fp32_product_zeros(o)
        assert zeros >= 1 and rows >= 1, (L, zeros, rows)
