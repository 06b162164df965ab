"""tests/logab_sweep.py draws its cases in a fixed order: the cases the GPU suite pins stay what they are
(tests/test_oneway_certificates_gpu.py).  No GPU needed."""
import numpy as np

import logab_sweep


def cases(seed, Q, n):
    rng = np.random.default_rng(seed)
    return [logab_sweep.make_case(rng, Q) for _ in range(n)]


def test_two_copy_seed1_case5_is_the_known_failure():
    """Seed 1, case 5 at Q = 29: b = 2, L = 700, forced chunk 48, six stretches — the log-likelihood that was off by
    1.1 nat on the 29-state model's one-directional entry points."""
    A = logab_sweep.gene_model(2)
    assert A.shape == (29, 29)
    b, L, chunk, E, nst = cases(1, 29, 6)[5]
    assert (b, L, chunk, nst) == (2, 700, 48, 6)
    assert E.shape == (2, 700, 29) and E.dtype == np.float32
    # a state emits alone for several positions somewhere in it: rows with exactly one nonzero emission
    assert ((E > 0).sum(-1) == 1).any()


def test_case_draws_are_pinned():
    assert [c[:3] + (c[4],) for c in cases(1, 29, 6)] == [
        (3, 9000, 48, 8), (1, 3000, 0, 0), (3, 20000, 48, 8), (1, 9000, 0, 4), (5, 700, 16, 5), (2, 700, 48, 6)]
    assert [c[:3] + (c[4],) for c in cases(0, 43, 3)] == [(6, 9000, 16, 9), (5, 3000, 16, 10), (5, 3000, 0, 3)]
    assert [c[:3] + (c[4],) for c in cases(0, 57, 3)] == [(6, 9000, 16, 7), (5, 20000, 0, 8), (4, 3000, 16, 8)]
    # the same stream gives the same emissions
    e1, e2 = cases(1, 29, 6)[5][3], cases(1, 29, 6)[5][3]
    assert np.array_equal(e1, e2)


def test_sweep_models_have_the_stated_sizes():
    assert logab_sweep.A15_DEFAULT.shape[0] in (15, 29, 43, 57)
    for k, q in ((2, 29), (3, 43), (4, 57)):
        A = logab_sweep.gene_model(k)
        assert A.shape == (q, q)
        assert np.allclose(A.sum(-1), 1.0, atol=1e-5)
