"""The sparse reduce with a step's emission row spread over the four lanes of a DPP quad (HMM_RS_QUADROW) and the
column sum formed only when some column's largest live entry is small (HMM_RS_SUMGATE): unit-weight 15-state gene
model, one model per wave.  The shapes are the smallest at which a broadcast source, the row carried from one
16-step tile to the next, the per-lane first steps of a chunk or the gate can go wrong.  The engine ships with the
gate on and the quad row off (it does not pay); the cases hold for either setting of either
switch and have been run with both on.

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
LIVE15 = list(range(0, 7))
PASS15 = list(range(7, 15))


def dev(x):
    return torch.as_tensor(np.asarray(x), dtype=torch.float32, device=DEV)


def check(A, pi, E, chunk, tag, after_sparse=None):
    """A (k,q,q), pi (k,q), E (k,b,L,q); after_sparse() runs right after the sparse-reduce call."""
    k = A.shape[0]
    got = []
    for dense in (0, 1):
        with engine.option(engine.OPT_CHUNK, chunk), engine.option(engine.OPT_FORCE_DENSE, dense):
            g, ll = engine.posterior(dev(A), dev(pi), dev(E))
            torch.cuda.synchronize()
            if dense == 0 and after_sparse is not None:
                after_sparse()
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


def gene15():
    return params.intended_A15().numpy()[None]


@pytest.mark.parametrize("L", [1, 2, 3, 15, 16, 17, 31, 32, 33, 48])
def test_first_steps_tile_boundaries_and_short_last_chunks(L):
    """Chunks of one 16-step tile.  L = 1, 2, 3 end inside or right after a chunk's two per-lane steps, 17 and 33
    one step into a last chunk, 15 and 31 one step short of a whole tile; 16, 32 and 48 are whole chunks."""
    rng = np.random.default_rng(700 + L)
    E = (rng.random((1, 3, L, 15)) * 0.9 + 0.05).astype(np.float32)
    check(gene15(), rand_pi(rng, 15)[None], E, 16, "L=%d" % L)


def test_rows_carried_across_tiles_of_one_chunk():
    """Chunks of 32 and 48 steps: two and three tiles per chunk, the odd row set carried from tile to tile."""
    rng = np.random.default_rng(707)
    E = (rng.random((1, 3, 100, 15)) * 0.9 + 0.05).astype(np.float32)
    for chunk in (32, 48):
        check(gene15(), rand_pi(rng, 15)[None], E, chunk, "chunk=%d" % chunk)


def test_every_broadcast_source():
    """State j's emission is (j+1)/16 times a number in [0.5, 1): taking any value from another quad lane or
    component is an error of at least 1/16 of the value."""
    rng = np.random.default_rng(710)
    u = rng.random((1, 3, 40, 15)) * 0.5 + 0.5
    E = (u * (np.arange(15) + 1) / 16.0).astype(np.float32)
    check(gene15(), rand_pi(rng, 15)[None], E, 16, "broadcast sources")


@pytest.mark.parametrize("state", range(15))
def test_start_distribution_on_each_state(state):
    """pi on one state: on a pass-through state the sequence-start step leaves the mass in flight with weight e0,
    seen by one lane only (the per-lane form of steps 0 and 1)."""
    rng = np.random.default_rng(720 + state)
    pi = np.full(15, 1e-6, dtype=np.float32)
    pi[state] = 1.0
    pi /= pi.sum()
    E = (rng.random((1, 3, 20, 15)) * 0.9 + 0.05).astype(np.float32)
    check(gene15(), pi[None], E, 16, "pi on state %d" % state)


def test_gate_live_part_small_while_mass_is_in_flight():
    """On every second step the live states emit 1e-13 and the pass-through states 0.9: the largest live entry of
    a column falls below the threshold while most of its sum is on the pass-through states."""
    rng = np.random.default_rng(730)
    E = (rng.random((1, 3, 200, 15)) * 0.9 + 0.05).astype(np.float32)
    E[:, :, 1::2, :7] = 1e-13
    E[:, :, 1::2, 7:] = 0.9
    check(gene15(), rand_pi(rng, 15)[None], E, 0, "gate, live part small")


def test_gate_rescales_and_clamps_with_mass_in_flight():
    """Small emissions with exact zeros on states 6-14 (tests/test_reduce_order2_gpu.py's ragged case): the gate
    opens every few steps, and the eps clamp meets the folded weight."""
    rng = np.random.default_rng(4 * 7919 + 600)
    E = (rng.random((4, 600, 15)) * 0.9 + 0.05).astype(np.float32) / 4096
    dead = rng.random(E.shape) < 0.5
    dead[..., :6] = False
    E[dead] = 0.0
    check(gene15(), rand_pi(rng, 15)[None], E[None], 0, "ragged emissions")


@pytest.mark.parametrize("state", [0, 3, 9])
def test_dead_columns(state):
    """30 rows that only one state can emit: the columns of most start states lose everything but floor-level
    mass and some underflow to exactly zero; such a lane sends its wave through the full sum every time and must
    change nothing else."""
    rng = np.random.default_rng(740 + state)
    A = gene15()
    pi = rand_pi(rng, 15)
    E = (rng.random((1, 3, 64, 15)) * 0.9 + 0.05).astype(np.float32)
    keep = E[:, :, :30, state].copy()
    E[:, :, :30, :] = 0.0
    E[:, :, :30, state] = keep
    g64, ll64 = textbook.posterior(A[0], pi, E[0])            # the oracle alone, before anything runs on the GPU
    assert np.isfinite(g64).all() and np.isfinite(ll64).all()
    assert np.abs(g64.sum(-1) - 1.0).max() <= 1e-9
    check(A, pi[None], E, 16, "dead columns, state %d" % state)


def test_two_floor_only_rows_in_a_row():
    """Rows 20 and 21 of one sequence are all zero: every path survives them at the emission floor only, the
    column goes through the denormal range between two sums and the chain is marked (risk): with OPT_EXACT at its
    default the sequence leaves the scan."""
    rng = np.random.default_rng(750)
    E = (rng.random((1, 3, 64, 15)) * 0.9 + 0.05).astype(np.float32)
    E[0, 1, 20:22, :] = 0.0
    det = {}

    def routed():
        det.update(engine.exact_detail((1, 3, 64, 15)))

    check(gene15(), rand_pi(rng, 15)[None], E, 16, "two floor rows", after_sparse=routed)
    print("two floor rows:", det)
    assert det["routed"] >= 1, det


def test_two_models_in_one_wave_keep_the_per_lane_step():
    """k = 2 gene models with different weights, 3 sequences of 3 chunks each: 9 chains per model, so the wave
    of chains 8-11 straddles the two models and takes the per-lane-weights, first-order path, which has neither
    the quad row nor the gate."""
    rng = np.random.default_rng(760)
    A = np.stack([params.intended_A15().numpy(), params.intended_A15(50, 300, 900).numpy()])
    assert ((A[0] != 0) == (A[1] != 0)).all() and not np.array_equal(A[0], A[1])
    pi = np.stack([rand_pi(rng, 15), rand_pi(rng, 15)])
    E = (rng.random((2, 3, 40, 15)) * 0.9 + 0.05).astype(np.float32)
    check(A, pi, E, 16, "two models")
