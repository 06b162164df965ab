"""The sparse reduce's second-order recurrence (HMM_RS_ORDER2): the pass-through states of the gene topologies
(START, EI, IE, STOP: one edge in, one edge out with weight 1) are never formed inside the step loop, their
incoming weight is folded into the staged emission, and mass that sits on one of them at a chunk's start or
end is "in flight".  The shapes are the smallest at which a two-step pipeline can go wrong.

Every case against the fp64 oracle (oracle.textbook.posterior) at the project's tolerances
    |gamma - gamma64| <= 2e-5,   |ll - ll64| <= 1e-6 |ll64|
and against the forced-dense reduce (two implementations of the same chunk operators) at those of
test_engine_gpu.py::test_sparse_and_dense_reduce_agree
    |gamma_sparse - gamma_dense| <= 2e-6,   |ll_sparse - ll_dense| <= 1e-7 |ll_dense|."""
import numpy as np
import pytest
import torch

from hmm_layer_amd import engine
from oracle import params, textbook

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
START = 7                   # a pass-through state of the 15-state model
PASS15 = list(range(7, 15))


def dev(x):
    return torch.as_tensor(np.asarray(x), dtype=torch.float32, device=DEV)


def check(A, pi, E, chunk, tag):
    """A (k,q,q), pi (k,q), E (k,b,L,q)."""
    k = A.shape[0]
    got = []
    for dense in (0, 1):
        with engine.option(engine.OPT_CHUNK, chunk), engine.option(engine.OPT_FORCE_DENSE, dense):
            g, ll = engine.posterior(dev(A), dev(pi), dev(E))
            torch.cuda.synchronize()
        got.append((g.cpu().numpy(), ll.cpu().numpy()))
    (g1, l1), (g2, l2) = got
    assert np.isfinite(g1).all() and np.isfinite(l1).all(), tag
    for m in range(k):
        g64, ll64 = textbook.posterior(A[m], pi[m], E[m])
        gerr = float(np.abs(g1[m] - g64).max())
        lerr = float(np.abs((l1[m] - ll64) / ll64).max())
        gd = float(np.abs(g1[m] - g2[m]).max())
        ld = float(np.abs((l1[m] - l2[m]) / l2[m]).max())
        print("%s model %d: vs fp64 gamma %.3g loglik rel %.3g; vs dense reduce gamma %.3g loglik rel %.3g"
              % (tag, m, gerr, lerr, gd, ld))
        assert gerr <= 2e-5, (tag, m, gerr)
        assert lerr <= 1e-6, (tag, m, lerr)
        assert gd <= 2e-6, (tag, m, gd)
        assert ld <= 1e-7, (tag, m, ld)


def rand_pi(rng, q):
    pi = rng.random(q).astype(np.float32) + 0.1
    return pi / pi.sum()


@pytest.mark.parametrize("L", [1, 2, 3, 16, 17, 18, 31, 33])
def test_short_sequences_and_short_last_chunks(L):
    """Chunks of 16: last chunks of length 1 and 2 end with mass still in flight, a first chunk of length 1
    ends on the sequence-start step."""
    rng = np.random.default_rng(200 + L)
    A = params.intended_A15().numpy()
    E = (rng.random((1, 3, L, 15)) * 0.9 + 0.05).astype(np.float32)
    check(A[None], rand_pi(rng, 15)[None], E, 16, "L=%d" % L)


@pytest.mark.parametrize("state", [START, 0])
def test_start_distribution_on_one_state(state):
    """pi concentrated on a pass-through state (the sequence-start step leaves its mass in flight) and on a live one."""
    rng = np.random.default_rng(300 + state)
    A = params.intended_A15().numpy()
    pi = np.full(15, 1e-6, dtype=np.float32)
    pi[state] = 1.0
    pi /= pi.sum()
    E = (rng.random((1, 3, 40, 15)) * 0.9 + 0.05).astype(np.float32)
    check(A[None], pi[None], E, 16, "pi on state %d" % state)


def test_rescales_and_clamps_with_mass_in_flight():
    """Small emissions with exact zeros on states 6-14: the column is rescaled every few steps while mass is in
    flight, and the eps clamp meets the folded weight."""
    rng = np.random.default_rng(4 * 7919 + 600)
    A = params.intended_A15().numpy()
    E = (rng.random((4, 600, 15)) * 0.9 + 0.05).astype(np.float32) / 4096
    dead = rng.random(E.shape) < 0.5
    dead[..., :6] = False
    E[dead] = 0.0
    check(A[None], rand_pi(rng, 15)[None], E[None], 0, "ragged emissions")


def test_non_unit_out_edges_take_the_first_order_step():
    """A gene-topology matrix whose pass-through rows are 0.999, not 1: not a pure delay any more."""
    rng = np.random.default_rng(400)
    A = params.intended_A15().numpy().copy()
    assert all((A[p] != 0).sum() == 1 and A[p].max() == 1.0 for p in PASS15)
    A[PASS15] *= np.float32(0.999)
    E = (rng.random((1, 3, 40, 15)) * 0.9 + 0.05).astype(np.float32)
    check(A[None], rand_pi(rng, 15)[None], E, 16, "non-unit")


def test_two_models_in_one_wave():
    """k = 2 gene models with different weights, 3 sequences of 3 chunks each: 9 chains per model, so the wave
    of chains 8-11 straddles the two models and takes the per-lane-weights path."""
    rng = np.random.default_rng(500)
    A = np.stack([params.intended_A15().numpy(), params.intended_A15(50, 300, 900).numpy()])
    assert ((A[0] != 0) == (A[1] != 0)).all() and not np.array_equal(A[0], A[1])
    pi = np.stack([rand_pi(rng, 15), rand_pi(rng, 15)])
    E = (rng.random((2, 3, 40, 15)) * 0.9 + 0.05).astype(np.float32)
    check(A, pi, E, 16, "two models")


def test_two_copy_29_state_model():
    """The 29-state two-copy model: 16 pass-through states, 13 live ones, 32 lanes per chain."""
    from hmm_layer_amd.gene_pred_hmm_transitioner import GenePredMultiHMMTransitioner
    tr = GenePredMultiHMMTransitioner(k=2, initial_exon_len=200, initial_intron_len=4500, initial_ir_len=10000)
    with torch.no_grad():
        A = tr.make_A()[0].numpy().copy()
        pi = tr.make_initial_distribution().reshape(-1).numpy().copy()
    assert A.shape == (29, 29) and (A > 0).sum() == 45
    rng = np.random.default_rng(600)
    E = (rng.random((1, 2, 100, 29)) * 0.9 + 0.05).astype(np.float32)
    check(A[None], pi[None], E, 16, "gene29")
