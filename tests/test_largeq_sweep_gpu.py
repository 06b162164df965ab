"""hmm_forward / hmm_backward / hmm_posterior above 64 states (hmm_largeq.inc) against the fp64 oracle: the randomised
sweep of tests/largeq_sweep.py (N = 64 cases of seed 239, the first seed whose 64 shapes meet the coverage conditions
that tests/test_largeq_sweep_cpu.py asserts) and the cases a random draw cannot be relied on to hit: the largest state
counts (the partial-sum row exactly full), the 80- and 96-column GEMM tiles with a ragged tile map, the five-copy gene
model over 4000 positions with the emitter's share of exact zeros, writes outside the output tensor, repeatability.

Every case goes through largeq_sweep.check_case: the three posterior modes, log alpha, log beta and the log-likelihood
of every entry point against oracle.textbook in fp64 at the tolerances of tests/test_engine_gpu.py, no NaN or +inf
anywhere, k >= 2 calls bitwise equal to the k = 1 calls.  Needs an MI355X.

Measured on an MI355X with 16 CPU threads: 8 s for this file (the sweep 4.3 s), against a budget of ten minutes;
nearly all of it is the fp64 oracle and the comparisons.  The long five-copy case (b = 3, 47 % zeros): 385 846 -inf
entries in the two log modes together at L = 4000 and 381 942 at L = 4001 (of 2 x 852 000 and 2 x 852 213; the CPU
emulation of tests/test_largeq_sweep_cpu.py predicts 2 x 192 923 and 2 x 190 971): the fp32 product U_t * Rb_t
underflows there, gamma64 at those entries is below the 2e-5 tolerance."""
import numpy as np
import pytest
import torch

import largeq_sweep as sweep
from hmm_layer_amd import engine
from largeq_sweep import N_CASES, SEED, long_five_copy_case, lq_tile_width, make_case
from oracle import build as obuild

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(x):
    return torch.as_tensor(np.asarray(x), dtype=torch.float32, device=DEV)


def sparse_diag_models(rng, k, q):
    """k different models as rand_model(dense=False) of tests/test_engine_gpu.py, built in float32 (q up to 4096)."""
    As, pis = [], []
    for _ in range(k):
        A = rng.random((q, q), dtype=np.float32) ** 3 + np.float32(1e-3)
        A *= rng.random((q, q), dtype=np.float32) < 0.3
        A[np.arange(q), np.arange(q)] += 0.5
        A /= A.sum(-1, keepdims=True)
        pi = rng.random(q) + 0.1
        As.append(A)
        pis.append((pi / pi.sum()).astype(np.float32))
    return np.stack(As), np.stack(pis)


def emissions(rng, shape, zero=0.1):
    E = (rng.random(shape) * 0.9 + 0.05).astype(np.float32)
    E[rng.random(shape) < zero] = 0.0
    return E


def checked(case, tag):
    fails, fig = sweep.check_case(case, tag)
    print(tag, {n: (v if isinstance(v, int) else float("%.3g" % v)) for n, v in fig.items()})
    assert not fails, fails[:10]
    return fig


def test_random_sweep():
    assert sweep.run(N_CASES, SEED) == 0


@pytest.mark.parametrize("q", [4096, 4095])
def test_largest_state_counts(q):
    """q = 4096 with 64-column tiles fills the LQ_NTP = 64 partial row sums of a row exactly; two models, so the second
    model's partial sums start right behind a full row.  q = 4095: the same with a ragged last tile and K slab."""
    b, L, k = 2, 3, 2
    assert engine.lib().hmm_max_states() == 4096
    assert engine.largeq_tile_cols(b, q) == 64 and lq_tile_width(b, q) == 4 and -(-q // 64) == 64
    rng = np.random.default_rng(q)
    A, pi = sparse_diag_models(rng, k, q)
    checked(make_case(A, pi, emissions(rng, (k, b, L, q))), "q=%d" % q)


def test_one_state_more_than_the_limit_raises():
    q = engine.lib().hmm_max_states() + 1
    with pytest.raises(ValueError, match="exceeds"):
        engine.posterior(torch.zeros((1, q, q), device=DEV), torch.zeros(q, device=DEV), torch.zeros((1, 2, 3, q), device=DEV))
    with pytest.raises(ValueError, match="exceeds"):
        engine.forward(torch.zeros((1, q, q), device=DEV), torch.zeros(q, device=DEV), torch.zeros((1, 2, 3, q), device=DEV))
    with pytest.raises(ValueError, match="exceeds"):
        engine.backward(torch.zeros((1, q, q), device=DEV), torch.zeros((1, 2, 3, q), device=DEV))


@pytest.mark.parametrize("b,q,L,ntw", [(300, 3375, 3, 5), (321, 3500, 2, 6)])
def test_wide_tiles_with_a_ragged_tile_map(b, q, L, ntw):
    """The 80- and 96-column instantiations where the XCD tile map has empty slots on both axes: MT = ceil(b/64) = 5, 6
    (not a multiple of 4), an odd number of tile columns (43, 37), q % 16 != 0, b % 64 != 0.  Every sequence and every
    output against the fp64 oracle (numpy; the C oracle on three sequences as a second opinion on gamma and loglik)."""
    mt, nt = -(-b // 64), -(-q // (16 * ntw))
    assert lq_tile_width(b, q) == ntw and mt % 4 != 0 and nt % 2 == 1 and q % 16 != 0
    assert engine.largeq_tile_cols(b, q) == 16 * ntw
    rng = np.random.default_rng(b + q)
    A, pi = sparse_diag_models(rng, 1, q)
    E = emissions(rng, (1, b, L, q))
    checked(make_case(A, pi, E), "b=%d q=%d" % (b, q))
    idx = [0, 63, b - 1]
    g64, ll64 = obuild.posterior(A[0], pi[0], E[0, idx])
    out, ll = engine.posterior(dev(A), dev(pi), dev(E))
    assert np.abs(out[0, idx].cpu().numpy() - g64).max() <= 2e-5
    assert np.all(np.abs(ll[0, idx].cpu().numpy() - ll64) <= 1e-6 * np.abs(ll64) + 2e-4)


@pytest.mark.parametrize("L", [4000, 4001])
def test_five_copy_gene_model_long(L):
    """The 71-state model over an even and an odd long L (the hand-over of the posterior's two recursions at
    h = (L+1)/2, thousands of ping-pong steps), 47 % exact zeros: the regime in which k_lq_normalise takes logf(0).
    The -inf count of the log modes must be positive: it proves the regime was reached
    (tests/test_largeq_sweep_cpu.py shows beforehand that it can be)."""
    fig = checked(long_five_copy_case(L), "five-copy L=%d" % L)
    assert fig["neginf"] > 0


def test_log_no_ll_is_rounded_once():
    """Pinned from the sweep (seed 239, case 45): a ring of 68 states, one sequence of 3000 positions, 47 % zeros, so
    that |loglik| = 8.4e3 lies above 8192 (fp32 ulp 9.8e-4).  k_lq_normalise added log g - log sum g + loglik in float,
    three roundings of that size: POST_LOG_NO_LL minus loglik was off by up to 1.35e-3 from log gamma64 where
    gamma64 > 1e-4, against the 1e-3 the log modes are held to.  It now adds in double and rounds once."""
    q, L = 68, 3000
    rng = np.random.default_rng(45)
    A = sweep.draw_model(rng, "ring", q, 0)
    pi = rng.random(q) + 0.1
    E = emissions(rng, (1, 1, L, q), zero=0.47)
    case = make_case(A[None], (pi / pi.sum())[None], E, kind="ring")
    ll64 = sweep.oracle(case["A"][0], case["pi"][0], case["E"][0], case["eps"])["ll"]
    assert 8192 < np.abs(ll64).min() and np.abs(ll64).max() < 16384
    fig = checked(case, "ring L=%d" % L)
    assert fig["lognoll_logspace"] <= 1e-3


def test_nothing_is_written_outside_the_output_tensor():
    """posterior(out=view) with the view a window of a larger buffer filled with a sentinel: q = 67, b = 65 is ragged in
    every tile dimension, k = 2 applies the per-model row offsets."""
    k, b, L, q, margin, sentinel = 2, 65, 7, 67, 1031, -12345.0
    rng = np.random.default_rng(67)
    A, pi = sparse_diag_models(rng, k, q)
    E = emissions(rng, (k, b, L, q))
    n = k * b * L * q
    for mode in (engine.POST_PROB, engine.POST_LOG, engine.POST_LOG_NO_LL):
        buf = torch.full((n + 2 * margin,), sentinel, device=DEV)
        view = buf[margin:margin + n].view(k, b, L, q)
        out, _ = engine.posterior(dev(A), dev(pi), dev(E), mode=mode, out=view)
        torch.cuda.synchronize()
        assert out.data_ptr() == view.data_ptr()
        assert bool((buf[:margin] == sentinel).all()) and bool((buf[margin + n:] == sentinel).all()), mode
        assert not bool((view == sentinel).any()), mode
        ref, _ = engine.posterior(dev(A), dev(pi), dev(E), mode=mode)
        assert torch.equal(ref, view), mode


def test_repeatable_and_stream_independent():
    q, b, L = 193, 65, 65
    rng = np.random.default_rng(193)
    A, pi = sparse_diag_models(rng, 1, q)
    A, pi, E = dev(A), dev(pi), dev(emissions(rng, (1, b, L, q)))

    def everything():
        res = []
        for mode in (engine.POST_PROB, engine.POST_LOG, engine.POST_LOG_NO_LL):
            res += list(engine.posterior(A, pi, E, mode=mode))
        res += list(engine.forward(A, pi, E))
        res.append(engine.backward(A, E))
        return res

    first, second = everything(), everything()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        third = everything()
    s.synchronize()
    for x, y, z in zip(first, second, third):
        assert torch.equal(x, y) and torch.equal(x, z)
