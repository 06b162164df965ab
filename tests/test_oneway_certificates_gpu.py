"""The one-directional entry points for 17..64 states in the eps-clamp regime: hmm_forward (log alpha with its
log-likelihood, and the log-likelihood alone) and hmm_backward (log beta) on the chunked 32- and 64-state scans.

The chunk operators are exactly linear; the cell clamps the predicted state mixture at eps every step
(hmm_layer/MsaHmmCell.py:87-88).  Where that clamp decides the answer, a sequence has to leave the chunked scan for the
serial kernels: per sequence, on the device, from the clamp-born share each entry point's apply kernel sums
(k32_forward / k64_forward's CERT, k32_backward / k64_backward's CERT3), or from the dense reduces' per-chain mark (the
operator columns went through the denormal range).  Every case here is held to the fp64 oracle (oracle/textbook.py)
at the suite's tolerances, every component in probability space, and the routing itself is checked: the sequences the
clamp decides are counted (engine.exact_count), and in the same call every other sequence is bit-identical to the
chunked scan alone (OPT_EXACT = EXACT_OFF) — routing everything to the serial kernels does not pass.
"""
import numpy as np
import pytest

from hmm_layer_amd import engine
from oracle import textbook

import logab_sweep
from test_engine_gpu import assert_log_close_in_probability_space, dev, rand_model

pytestmark = pytest.mark.gpu

LL_TOL = (1e-6, 2e-4)                        # |ll - ll64| <= 1e-6 |ll64| + 2e-4, the suite's log-likelihood bound


def gene_A(k):
    return logab_sweep.gene_model(k)


# ---- the randomised sweep (tests/logab_sweep.py), per model

@pytest.mark.parametrize("k,seed,ncase", [(0, 11, 12), (2, 0, 12), (3, 0, 12), (4, 0, 10)])
def test_sweep(k, seed, ncase):
    """Random local stretches (a state emitting alone, nothing emitting, dead columns) at forced chunk lengths:
    the 15-state model (k = 0) and GenePredMultiHMMTransitioner(k) with 29, 43 and 57 states."""
    A = logab_sweep.A15_DEFAULT if k == 0 else gene_A(k)
    assert logab_sweep.run(ncase, seed, A, verbose=True) == 0


def test_sweep_pinned_two_copy_cases():
    """Seed 1, cases 0..5 of the 29-state model: case 5 (b = 2, L = 700, chunk 48, six stretches; pinned on the CPU
    by tests/test_oneway_cases_cpu.py) was a log-likelihood off by 1.1 nat and log alpha off by 0.84 in probability
    space — a state emitting alone for several positions that some operator columns survive."""
    assert logab_sweep.run(6, 1, gene_A(2), verbose=True) == 0


# ---- constructed inputs

def outputs(A, pi, E):
    """The three one-directional calls on (k, b, L, q) input -> (log alpha, log-likelihood with it, log-likelihood
    alone, log beta) as numpy arrays, and the number of sequences each call sent to the serial kernels."""
    k, b, L, q = E.shape
    dims = (k, b, L, q)
    la, ll = engine.forward(dev(A), dev(pi), dev(E))
    n_fwd = engine.exact_count(engine.OP_FORWARD, dims)
    _, llo = engine.forward(dev(A), dev(pi), dev(E), want_log_alpha=False)
    n_ll = engine.exact_count(engine.OP_LOGLIK, dims)
    lb = engine.backward(dev(A), dev(E))
    n_bwd = engine.exact_count(engine.OP_BACKWARD, dims)
    res = tuple(x.cpu().numpy() for x in (la, ll, llo, lb))
    return res, (n_fwd, n_ll, n_bwd)


def check_oneway(A, pi, E, tag, must, maybe=(), routed_models=(), ll_may_stay=()):
    """A (k,q,q), pi (k,q), E (k,b,L,q).  Every output against the fp64 oracle; the routing: in model 0 the sequences
    `must` (and possibly `maybe`) leave the chunked scan, the others are bit-identical to EXACT_OFF; the models in
    `routed_models` are served by the serial kernels whole.  ll_may_stay: sequences of `must` that the log-likelihood
    alone may keep on the chunked scan — log alpha carries the clamp-born share of the filtered vector itself, the
    log-likelihood only the posterior mass of clamp-born paths (its value is held to the oracle all the same)."""
    k, b, L, q = E.shape
    (la, ll, llo, lb), counts = outputs(A, pi, E)
    for m in range(k):
        la64, ll64 = textbook.log_alpha(A[m], pi[m], E[m])
        lb64 = textbook.log_beta(A[m], E[m])
        t = "%s model %d" % (tag, m)
        assert np.isfinite(la[m]).all() and np.isfinite(lb[m]).all(), t
        assert_log_close_in_probability_space(la[m], la64, t + " log alpha")
        assert_log_close_in_probability_space(lb[m], lb64, t + " log beta")
        bound = LL_TOL[0] * np.abs(ll64) + LL_TOL[1]
        assert np.all(np.abs(ll[m] - ll64) <= bound), (t, "log-likelihood with log alpha", ll[m] - ll64)
        assert np.all(np.abs(llo[m] - ll64) <= bound), (t, "log-likelihood alone", llo[m] - ll64)
    with engine.option(engine.OPT_EXACT, engine.EXACT_OFF):
        (la0, ll0, llo0, lb0), counts0 = outputs(A, pi, E)
    assert counts0 == (0, 0, 0), (tag, counts0)
    for name, got, off, n in (("log alpha", la, la0, counts[0]), ("log-likelihood alone", llo, llo0, counts[1]),
                              ("log beta", lb, lb0, counts[2])):
        need = set(must) - (set(ll_may_stay) if got is llo else set())
        moved = [s for s in range(b) if not np.array_equal(got[0, s], off[0, s])]
        assert need <= set(moved) <= set(must) | set(maybe), (tag, name, moved, must)
        assert n == len(moved) + b * len(routed_models), (tag, name, n, moved)
    return counts


def cyclic(q):
    """A cycle with one self loop: primitive, with the longest possible index — mass moves on by one state per step,
    so a stretch that only one state can emit is survived through the eps clamps alone."""
    A = np.roll(np.eye(q, dtype=np.float32), 1, axis=1)
    A[0, 0] = 0.5
    A[0, 1] = 0.5
    return A


def uniform(q):
    return np.full(q, 1 / q, dtype=np.float32)


def test_scan64_routing_input_every_entry_point():
    """The input of test_scan64_gpu.py::test_routing_per_model_per_sequence_and_by_batch_size: the cyclic 43-state
    model with state 20 emitting alone for t = 300..329 (exactly one operator column keeps its mass at each step: no
    reduce mark), and a reducible model in the same call."""
    rng = np.random.default_rng(9)
    q, b, L = 43, 3, 900
    A1 = np.triu(rand_model(rng, q)[0])
    A1 /= A1.sum(-1, keepdims=True)
    E = (rng.random((2, b, L, q)) * 0.9 + 0.05).astype(np.float32)
    E[0, 1, 300:330] = 0.0
    E[0, 1, 300:330, 20] = 0.5
    A = np.stack([cyclic(q), A1.astype(np.float32)])
    pi = np.stack([uniform(q), uniform(q)])
    check_oneway(A, pi, E, "cyclic 43 + reducible", must=[1], routed_models=[1])


@pytest.mark.parametrize("q,kind", [(29, "cyclic"), (24, "dense")])
def test_state_alone_on_the_32_state_path(q, kind):
    """The same construction on the 32-state path: a cyclic 29-state model (outside the compiled gene topology: the
    dense reduce), and a dense 24-state model (every state reaches state 20 in one step: the clamp need not decide)."""
    rng = np.random.default_rng(q)
    b, L = 3, 900
    A0 = cyclic(q) if kind == "cyclic" else rand_model(rng, q)[0]
    A1 = np.triu(rand_model(rng, q)[0])
    A1 /= A1.sum(-1, keepdims=True)
    E = (rng.random((2, b, L, q)) * 0.9 + 0.05).astype(np.float32)
    E[0, 1, 300:330] = 0.0
    E[0, 1, 300:330, 20] = 0.5
    A = np.stack([A0, A1.astype(np.float32)])
    pi = np.stack([uniform(q), uniform(q)])
    if kind == "cyclic":
        # (the log-likelihood alone: the scan's value is within the bound here, and its certificate says so)
        check_oneway(A, pi, E, "cyclic %d" % q, must=[1], routed_models=[1], ll_may_stay=[1])
    else:
        check_oneway(A, pi, E, "dense %d" % q, must=[], maybe=[1], routed_models=[1])


@pytest.mark.parametrize("q", [32, 64])
@pytest.mark.parametrize("kind", ["dense", "sparse", "cyclic"])
def test_exactly_32_and_64_states(q, kind):
    """Models that fill the 32- / 64-state tiles exactly (no pad lane in the exponent row).  Sequence 1: two
    consecutive observations that every state emits at the floor only (every operator column goes through the
    denormal range); sequence 2: one state emitting alone for 25 positions; sequence 0: nothing special."""
    rng = np.random.default_rng(1000 + q)
    b, L = 3, 700
    if kind == "cyclic":
        A = cyclic(q)
    else:
        A = rand_model(rng, q, dense=kind == "dense")[0]
    E = (rng.random((1, b, L, q)) * 0.9 + 0.05).astype(np.float32)
    E[0, 1, 400:402] = 0.0
    E[0, 2, 200:225] = 0.0
    E[0, 2, 200:225, 7] = 0.5
    must, maybe = ([1, 2], []) if kind == "cyclic" else ([1], [2])
    with engine.option(engine.OPT_CHUNK, 48):
        check_oneway(A[None], uniform(q)[None], E, "%s q=%d" % (kind, q), must=must, maybe=maybe)
