"""The wide Viterbi restatement (tests/viterbi_wide.py) against the oracles where those can check it, and the
host side of hmm_viterbi_large (no device needed)."""
import numpy as np
import pytest

from oracle import viterbi as ov
from tests import viterbi_wide as vw


@pytest.mark.parametrize("q,kind", [(3, "dense"), (15, "sparse"), (64, "band"), (100, "dense"), (127, "sparse")])
def test_restatement_matches_the_oracle_up_to_127_states(q, kind):
    rng = np.random.default_rng(q)
    logA, logpi = vw.random_model(rng, q, kind)
    for b, L in ((1, 1), (3, 2), (4, 23)):
        logE = vw.random_logE(rng, b, L, q)
        want = ov.viterbi(logA, logpi, logE)
        got = vw.viterbi(logA, logpi, logE, chunk=q * q)            # one sequence per block as well
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_restatement_ties_and_clamp():
    rng = np.random.default_rng(7)
    q = 40
    logA = np.full((q, q), np.log(1.0 / q), dtype=np.float32)
    logpi = np.full(q, np.log(1.0 / q), dtype=np.float32)
    logE = np.log(np.array([0.25, 0.5, 1.0], dtype=np.float32))[rng.integers(0, 3, (5, 30, q))]
    want = ov.viterbi(logA, logpi, logE)
    got = vw.viterbi(logA, logpi, logE)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    clampE = np.full((2, 20, q), -np.inf, dtype=np.float32)
    clampE[:, :, 5] = -3.0
    want = ov.viterbi(logA, logpi, clampE)
    got = vw.viterbi(logA, logpi, clampE)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


@pytest.mark.parametrize("seed", range(4))
def test_restatement_score_is_the_brute_force_optimum(seed):
    rng = np.random.default_rng(100 + seed)
    q, L = 3 + seed % 2, 5
    logA, logpi = vw.random_model(rng, q, "sparse" if seed % 2 else "dense")
    logE = vw.random_logE(rng, 1, L, q)
    path, score = vw.viterbi(logA, logpi, logE)
    assert score[0] == ov.brute_force(logA, logpi, logE[0])
    assert ov.path_score(logA, logpi, logE[0], path[0]) == score[0]


def test_restatement_is_exact_where_int8_backpointers_are_not():
    """Above 127 states the int8 oracle wraps its backpointers; the restatement's path still scores its score."""
    rng = np.random.default_rng(3)
    logA, logpi = vw.random_model(rng, 200, "band")
    logE = vw.random_logE(rng, 2, 12, 200)
    path, score = vw.viterbi(logA, logpi, logE)
    assert path.max() < 200 and path.min() >= 0
    for s in range(2):
        assert ov.path_score(logA, logpi, logE[s], path[s]) == score[s]


def test_large_entry_point_host_side():
    from hmm_layer_amd import build as hbuild
    from hmm_layer_amd import engine
    hbuild.build()
    lib = engine.lib()
    assert lib.hmm_viterbi_large_max_states() == 4096
    assert lib.hmm_viterbi_max_states() == 64
    assert engine.OPT_VLARGE == 7
    k, b, L, q = 2, 1024, 6, 1027
    need = lib.hmm_viterbi_large_workspace_bytes(k, b, L, q)
    assert need >= 2 * k * b * L * q and need - 2 * k * b * L * q < 2 * 4 * k * b * q + (1 << 20)
    assert lib.hmm_viterbi_large_workspace_bytes(1, 1, 1, 4097) == 0
    assert lib.hmm_viterbi_large_workspace_bytes(1, 1, 1, 1) > 0
    # more than 2^32 backpointer bytes: the size is computed in 64 bits
    assert lib.hmm_viterbi_large_workspace_bytes(1, 1024, 30000, 71) > 2 * 1024 * 30000 * 71
    assert lib.hmm_viterbi_large(None, None, None, 1, 1, 1, 4097, None, None, None, 0, None) == -2
    assert lib.hmm_viterbi_large(None, None, None, 1, 0, 1, 65, None, None, None, 0, None) == -1
    assert lib.hmm_viterbi_large(None, None, None, 1, 1, 1, 65, None, None, None, 0, None) == -3
    old = engine.set_option(engine.OPT_VLARGE, 2)
    assert engine.get_option(engine.OPT_VLARGE) == 2
    engine.set_option(engine.OPT_VLARGE, old)
