"""Models, emissions, class maps and bounds shared by the tests of hmm_posterior_walk / hmm_posterior_decode_wide
(65..256 states): tests/test_posterior_walk_cpu.py checks every label case's margin share on the fp64 oracle alone,
tests/test_posterior_walk_gpu.py runs the same cases on the device.

Bounds.  The walk's posteriors are held to the fp64 oracle with the numbers of tests/largeq_sweep.py (check_walk
below restates them).  The decoded output is held to fp64 class sums of the engine's own gamma with tol(n) of
tests/posterior_decode_mid_cases.py, and to the oracle with STATE_TOL per state; MARGIN_CAP and ORACLE_CAP are that
file's shares of positions that may lie within the margin of a tie.  Emissions of the label cases are that file's
peaked emissions()."""
import functools

import numpy as np

import largeq_sweep as lq
import posterior_decode_mid_cases as mid
from posterior_decode_mid_cases import MARGIN_CAP, ORACLE_CAP, STATE_TOL, emissions, gene_classes, largest_class, tol
from posterior_decode_mid_cases import random_map

T = 16                                     # WQ_T: gamma rows each half of the workgroup stages before a collapse
Q_MIN, Q_MAX, Q_REG = 65, 256, 128         # the walk's range; the dense step keeps A in registers up to Q_REG
STATES = (65, 71, 100, 127, 128, 129, 253, 256)
GENE_STATES = (71, 127, 253)               # 5, 9 and 18 copies
LENGTHS = (1, 2, 3, T - 1, T, T + 1, 2 * T + 1, 300)


# ---------------------------------------------------------------- models

def degree_model(rng, q, hubs):
    """Every state has exactly 7 + (hubs == 0) predecessors and as many successors (a circulant); then `hubs` states
    get two more predecessors each, from rows of their own, which makes them the only states above 8: 0 hubs is a
    model with exactly 8 everywhere (sparse step), 1 and 2 sit on the hub rule, 3 is past it (dense step)."""
    offs = np.arange(8 if hubs == 0 else 7)
    A = np.zeros((q, q))
    for d in offs:
        A[np.arange(q), (np.arange(q) + d) % q] = rng.random(q) + 0.2
    for h in range(hubs):
        hub = 5 + 20 * h
        for src in (hub + 10, hub + 13):                      # not among the circulant's predecessors hub-6 .. hub
            assert A[src % q, hub] == 0
            A[src % q, hub] = 0.5
    A /= A.sum(-1, keepdims=True)
    A = A.astype(np.float32)
    deg = np.maximum((A != 0).sum(0), (A != 0).sum(1))
    assert (deg > 8).sum() == hubs and deg.max() == (9 if hubs else 8)
    return A


def one_model(rng, kind, q, m=0):
    """-> A (q,q), pi (q,) float32.  kind: 'gene' (q = 1 + 14 copies), 'dense' (rand_model), 'deg0'..'deg3'
    (degree_model), or a kind of largeq_sweep.draw_model ('ring', 'identity', 'cycle', 'zero_absorb', 'sparse_diag')."""
    if kind in ("gene", "dense"):
        A, pi = mid.model(kind, q, 1, rng)
        return A[0], pi[0]
    if kind.startswith("deg"):
        A = degree_model(rng, q, int(kind[3:]))
    else:
        while True:
            A = lq.draw_model(rng, kind, q, m)
            if lq.model_is_usable(A):
                break
    pi = rng.random(q) + 0.1
    return A, (pi / pi.sum()).astype(np.float32)


def models(rng, kind, q, k):
    A, pi = zip(*(one_model(rng, kind, q, m) for m in range(k)))
    return np.stack(A), np.stack(pi)


# ---------------------------------------------------------------- 1. the walk against the fp64 oracle

def walk_cases():
    """-> list of (tag, kind, q, (k, b, L), zero fraction, blank position, eps).  Flat emissions 0.05 + 0.9 u as in
    largeq_sweep.draw_case, `zero` of them exact zeros, one all-zero position per sequence where `blank`."""
    c = [("gene71", "gene", 71, (2, 3, 300), 0.47, True, 1e-16),
         ("gene127", "gene", 127, (1, 5, 2 * T + 1), 0.0, False, 1e-16),
         ("gene253", "gene", 253, (1, 3, 300), 0.47, True, 1e-16),
         ("gene253-eps", "gene", 253, (2, 1, T + 1), 0.1, False, 1e-6),
         ("gene71-eps", "gene", 71, (1, 3, T), 0.3, True, 1e-6),
         ("dense65", "dense", 65, (2, 3, T - 1), 0.0, False, 1e-16),
         ("dense100", "dense", 100, (1, 5, 300), 0.47, True, 1e-16),
         ("dense100-eps", "dense", 100, (1, 3, 2 * T + 1), 0.3, False, 1e-6),
         ("dense128", "dense", 128, (1, 3, 2 * T + 1), 0.47, False, 1e-16),
         ("dense129", "dense", 129, (1, 3, 2 * T + 1), 0.1, True, 1e-16),
         ("dense256", "dense", 256, (1, 1, T + 1), 0.0, False, 1e-16),
         ("ring127", "ring", 127, (1, 3, 300), 0.1, False, 1e-16),
         ("identity128", "identity", 128, (1, 3, T), 0.0, False, 1e-16),
         ("cycle253", "cycle", 253, (2, 3, T + 1), 0.3, False, 1e-16),
         ("zero-rows100", "zero_absorb", 100, (2, 3, 2 * T + 1), 0.1, False, 1e-16),
         ("zero-rows200", "zero_absorb", 200, (1, 1, T - 1), 0.0, True, 1e-16)]
    for L in (1, 2, 3):
        c.append(("gene71-L%d" % L, "gene", 71, (1, 3, L), 0.3, False, 1e-16))
        c.append(("dense129-L%d" % L, "dense", 129, (1, 3, L), 0.0, False, 1e-16))
    for q in (96, 160):                                     # on the step rule: 8 everywhere, 1, 2, 3 states above 8
        for hubs in range(4):
            c.append(("deg%d-%d" % (hubs, q), "deg%d" % hubs, q, (1, 3, 2 * T + 1), 0.1, False, 1e-16))
    return c


@functools.lru_cache(maxsize=None)
def _walk_inputs(tag):
    case = next(c for c in walk_cases() if c[0] == tag)
    _, kind, q, (k, b, L), zero, blank, eps = case
    rng = np.random.default_rng([11, q, k, b, L, sum(map(ord, tag))])
    A, pi = models(rng, kind, q, k)
    E = (rng.random((k, b, L, q)) * 0.9 + 0.05).astype(np.float32)
    if zero > 0:
        E[rng.random(E.shape) < zero] = 0.0
    if blank:
        t0 = rng.integers(0, L, size=(k, b))
        for m in range(k):
            E[m, np.arange(b), t0[m]] = 0.0
    oracles = tuple(lq.oracle(A[m], pi[m], E[m], eps) for m in range(k))
    for x in (A, pi, E):
        x.flags.writeable = False
    return A, pi, E, eps, oracles


def walk_inputs(case):
    """-> A, pi, E, eps, (oracle of every model): computed once per case and shared, read-only."""
    return _walk_inputs(case[0])


def check_walk(got, o, tag):
    """The posterior checks of tests/largeq_sweep.py::check_model, the same numbers, for ONE model.  got: dict with
    prob, log, lognoll (b,L,q) and ll_prob, ll_log, ll_lognoll (b,); o: lq.oracle(...).  -> (failures, figures)."""
    fails, fig = [], {}
    g64, ll64 = o["g"], o["ll"]

    def need(ok, what, *val):
        if not ok:
            fails.append("%s: %s %s" % (tag, what, " ".join("%.3g" % v for v in val)))

    for name in ("prob", "log", "lognoll"):
        need(not np.isnan(got[name]).any(), name + " has NaN")
        need(not (got[name] == np.inf).any(), name + " has +inf")
    need(np.isfinite(got["prob"]).all(), "prob is not entirely finite")
    fig["rowsum"] = lq._mx(np.abs(got["prob"].sum(-1) - 1))
    need(fig["rowsum"] <= 2e-5, "rows of POST_PROB do not sum to 1:", fig["rowsum"])
    fig["prob"] = lq._mx(np.abs(got["prob"] - g64))
    need(fig["prob"] <= 2e-5, "POST_PROB", fig["prob"])
    m = g64 > 1e-4
    lg64 = np.log(np.maximum(g64, 1e-300))
    for name, sub, bound in (("log", 0.0, 2e-5),
                             ("lognoll", got["ll_lognoll"][:, None, None], 2e-5 + 2.4e-7 * np.abs(ll64).max())):
        with np.errstate(over="ignore", under="ignore", invalid="ignore"):
            lg = got[name] - sub
            fig[name] = lq._mx(np.abs(np.exp(lg) - g64))
            fig[name + "_logspace"] = lq._mx(np.abs(lg - lg64)[m])
        need(fig[name] <= bound, "exp(%s)" % name, fig[name], bound)
        need(fig[name + "_logspace"] <= 1e-3, "%s in log space" % name, fig[name + "_logspace"])
    for name in ("ll_prob", "ll_log", "ll_lognoll"):
        ex = lq._mx(np.abs(got[name] - ll64) - (1e-6 * np.abs(ll64) + 2e-4))
        fig["ll"] = max(fig.get("ll", -np.inf), ex)
        need(ex <= 0, name + " excess", ex)
        need(np.array_equal(got[name], got["ll_prob"]), name + " differs bitwise from POST_PROB's loglik")
    return fails, fig


# ---------------------------------------------------------------- 2. decoded output

def class_cases():
    """-> list of (tag, model kind, q, table, C, seed), inputs from class_inputs for every shape of CLASS_SHAPES:
    compared with fp64 class sums of the walk's own gamma."""
    rng = np.random.default_rng(3)
    c = [("gene%d-6" % q, "gene", q, gene_classes(q), 6, 100 + q) for q in GENE_STATES]
    for q, C in ((65, 5), (100, 16), (128, 1), (129, 5), (200, 16), (256, 16), (256, 5)):
        c.append(("dense%d-%d" % (q, C), "dense", q, random_map(rng, q, C), C, 200 + q + C))
    c.append(("dense100-empty", "dense", 100, random_map(rng, 100, 7, empty=(2, 5)), 7, 300))
    c.append(("gene71-empty0", "gene", 71, [x + 1 for x in gene_classes(71)], 7, 301))
    return c


CLASS_SHAPES = ((2, 3, 2 * T + 1), (1, 5, 130))             # (k, b, L)


def class_inputs(case, shape):
    tag, kind, q, table, C, seed = case
    k, b, L = shape
    rng = np.random.default_rng([seed, k, b, L])
    A, pi = mid.model(kind, q, k, rng)
    return A, pi, emissions(rng, k, b, L, q)


def oracle_cases():
    """-> list of (tag, kind, q, table or None, C, seed), inputs from oracle_inputs for every shape of ORACLE_SHAPES:
    labels compared with the fp64 oracle's.  Dense models of at most 129 states only: with 200 and 256 states and 16
    classes more than ORACLE_CAP of the positions lie within 2 n STATE_TOL of a tie."""
    rng = np.random.default_rng(5)
    c = []
    for q in GENE_STATES:
        c.append(("gene%d-6" % q, "gene", q, gene_classes(q), 6, 400 + q))
        c.append(("gene%d-ident" % q, "gene", q, None, q, 500 + q))
    for q, C in ((65, 4), (100, 16)):
        c.append(("dense%d-%d" % (q, C), "dense", q, random_map(rng, q, C), C, 600 + q))
    c.append(("dense129-ident", "dense", 129, None, 129, 729))     # (with 5 or 16 classes: 2.2 % within the margin)
    return c


ORACLE_SHAPES = ((1, 4, 300), (2, 3, 333))


@functools.lru_cache(maxsize=None)
def _oracle_inputs(tag, shape):
    case = next(c for c in oracle_cases() if c[0] == tag)
    A, pi, E = class_inputs(case, shape)
    from oracle import textbook
    post = [textbook.posterior(A[m], pi[m], E[m]) for m in range(E.shape[0])]
    g64, ll64 = np.stack([p[0] for p in post]), np.stack([p[1] for p in post])
    for x in (A, pi, E, g64, ll64):
        x.flags.writeable = False
    return A, pi, E, g64, ll64


def oracle_inputs(case, shape):
    """-> A, pi, E, gamma64 (k,b,L,q), ll64 (k,b): computed once per (case, shape) and shared, read-only."""
    return _oracle_inputs(case[0], shape)
