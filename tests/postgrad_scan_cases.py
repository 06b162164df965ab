"""Inputs of the tests of hmm_posterior_grad_scan (csrc/hmm_postgrad_scan.inc: the posterior gradients per chunk of the
scan plan for 17..64 states, rows of 32 lanes up to 32 states and of 64 above).

Test infrastructure; imports neither the engine nor a GPU.  The fp64 oracle, its fp32 twin and the four norms are those
of tests/postgrad_mid_cases.py.  tests/test_posterior_grad_scan_cpu.py proves from fp64 alone that the cases can carry
their assertions (primitive models, the per-chunk path's certificate far from firing where a case must be served, the
flagged case far above it); tests/test_posterior_grad_scan_gpu.py runs the kernels on them.

A case is a Case; build(case) -> dict(A (1,q,q), pi (1,q), E (1,b,L,q), G (1,b,L,q)) float32, read-only, the same
arrays in every process.  reference(case) -> dict(want, e32, limit, small) as postgrad_mid_cases.reference gives per
model, computed once.

  models     dense primitive: A = rand^2 + 1e-2 row-normalised, pi = rand + 0.1 normalised (no dead state, no tiny
             pi: a state nothing enters makes the support reducible, and k32_check / k64_check hand the model back);
             gene: the 29-, 43- and 57-state gene models with a random start distribution
  emissions  uniform in [0.05, 0.95]
  POST_PROB  G = randn; E = 0 at [:, ::9, 20 % q]: clamped emissions, dE there must be exactly 0
  POST_LOG   G = -onehot(argmax of the fp64 posterior), the cross-entropy against the most probable state; no holes
"""
import collections
import functools

import numpy as np
import torch

from postgrad_mid_cases import EPS, FINE_FACTOR, FINE_FLOOR, FINE_NORMS, errors, gene_model, limits, oracle  # noqa: F401

Case = collections.namedtuple("Case", "model q b L chunk log seed")

DENSE_Q = (17, 24, 32, 33, 48, 49, 64)
GENE_Q = (43, 57)
# (b, L, chunk): 21 chunks with a ragged last one; 5 x 7 chains, an odd count for the two-rows-per-wave width
SHAPES = ((3, 333, 16), (5, 97, 16))
HOLE_STEP = 9
PG_TINY_GAMMA = 1e-8                                         # csrc/hmm_postgrad.inc
EXACT_DELTA, PC_LOG_EXPOSED = 2e-6, 1e-4                     # csrc/hmm_engine.hip, csrc/hmm_postgrad_chunked.inc


def case_id(c):
    return "%s-q%d-b%d-L%d-T%d-%s" % (c.model, c.q, c.b, c.L, c.chunk, "log" if c.log else "prob")


# Cases whose default seed (1) does not meet the conditions of tests/test_posterior_grad_scan_cpu.py, with the first
# seed of 11, 21, ... that does (postgrad_mid_cases.SEEDS' convention).
SEEDS = {}


def seeded(cases):
    return [c._replace(seed=SEEDS.get(case_id(c), c.seed)) for c in cases]


def all_cases():
    out = []
    for log in (False, True):
        for b, L, T in SHAPES:
            out += [Case("dense", q, b, L, T, log, 1) for q in DENSE_Q]
            out += [Case("gene", q, b, L, T, log, 1) for q in GENE_Q]
        out += [Case("dense", q, 2, 700, 0, log, 1) for q in (32, 33, 64)]
        out += [Case("gene", 43, 2, 700, 0, log, 1), Case("gene", 43, 1, 2100, 64, log, 1)]
    out += [Case("gene", 29, 3, 333, 16, log, 1) for log in (False, True)]     # the compiled sparse reduce, once
    return seeded(out)


def dense_model(rng, q):
    A = rng.random((q, q)) ** 2 + 1e-2
    A /= A.sum(-1, keepdims=True)
    pi = rng.random(q) + 0.1
    pi /= pi.sum()
    return A.astype(np.float32), pi.astype(np.float32)


def model_of(rng, kind, q):
    if kind == "gene":
        pi = rng.random(q) + 0.1
        return np.array(gene_model((q - 1) // 14)[0]), (pi / pi.sum()).astype(np.float32)
    return dense_model(rng, q)


def recursions64(A, pi, E, eps=EPS):
    """The cell's two recursions in numpy fp64 -> gamma (b,L,q), Sg (b,L) = <alpha_hat_t, Rb_t>."""
    A, pi, E = np.asarray(A, np.float64), np.asarray(pi, np.float64), np.asarray(E, np.float64)
    b, L, q = E.shape
    Ec = np.maximum(E, eps)
    ah, Rb = np.empty((b, L, q)), np.empty((b, L, q))
    state = np.broadcast_to(np.maximum(pi, eps), (b, q))
    for t in range(L):
        R = state if t == 0 else np.maximum(state @ A, eps)
        sf = Ec[:, t] * R
        state = sf / sf.sum(-1, keepdims=True)
        ah[:, t] = state
    bh = None
    for t in range(L - 1, -1, -1):
        R = np.ones((b, q)) if t == L - 1 else np.maximum(bh @ A.T, eps)
        Rb[:, t] = R
        sb = Ec[:, t] * R
        bh = sb / sb.sum(-1, keepdims=True)
    g = ah * Rb
    Sg = g.sum(-1)
    return g / Sg[..., None], Sg


def certificate(A, pi, E, G, eps=EPS):
    """What k_pc_scan sums per sequence, in fp64: F = eps * sum_t 1 / Sg_t, and the share of sum |G| that is exposed to
    the floors in log mode, (F * sum_{gamma >= 1e-8} |G| / gamma + sum_{gamma < 1e-8} |G|) / sum |G|."""
    gam, Sg = recursions64(A, pi, E, eps)
    F = eps * (1.0 / Sg).sum(-1)
    w = np.abs(np.asarray(G, np.float64))
    tiny = gam < PG_TINY_GAMMA
    exposed = F * np.where(tiny, 0.0, w / np.where(tiny, 1.0, gam)).sum((1, 2)) + np.where(tiny, w, 0.0).sum((1, 2))
    return F, exposed / w.sum((1, 2))


def primitive_power(A):
    """The smallest n <= q^2 - 2q + 2 (Wielandt) with (A > 0)^n entrywise positive, or None."""
    S = np.asarray(A) > 0
    q = S.shape[0]
    P = S.copy()
    for n in range(1, q * q - 2 * q + 3):
        if P.all():
            return n
        P = (P.astype(np.int64) @ S.astype(np.int64)) > 0
    return None


def build(case):
    return _build(case)


@functools.lru_cache(maxsize=None)
def _build(case):
    q, b, L = case.q, case.b, case.L
    rng = np.random.default_rng([case.seed, q, b, L, int(case.log), 77])
    A, pi = model_of(rng, case.model, q)
    E = (rng.random((1, b, L, q)) * 0.9 + 0.05).astype(np.float32)
    if case.log:
        gam = recursions64(A, pi, E[0])[0]
        G = -(gam == gam.max(-1, keepdims=True)).astype(np.float32)[None]
    else:
        E[:, :, ::HOLE_STEP, 20 % q] = 0.0
        G = rng.standard_normal(E.shape).astype(np.float32)
    out = dict(A=A[None], pi=pi[None], E=E, G=G)
    for v in out.values():
        v.flags.writeable = False
    return out


@functools.lru_cache(maxsize=None)
def reference(case):
    """dict(want=(dA, dpi, dE) fp64, e32, limit, small) of the case's one model; computed once, read-only."""
    c = build(case)
    want = oracle(c["A"][0], c["pi"][0], c["E"][0], c["G"][0], case.log)
    twin = oracle(c["A"][0], c["pi"][0], c["E"][0], c["G"][0], case.log, torch.float32)
    for x in want:
        x.flags.writeable = False
    e32, small = errors(twin, want, c["A"][0])
    return dict(want=want, e32=e32, limit={n: max(FINE_FLOOR, FINE_FACTOR * e32[n]) for n in FINE_NORMS}, small=small)


# ---- the routing cases of the GPU test ----------------------------------------------------------------------------
# q = 43: seed 5 left one sequence with an exposed weight of 2e-5 of sum |G| (the draws vary between 1e-5 and 3e-2);
# 15 is the first of 5, 15, 25 with every sequence >= 1e-3 (2.5e-3 .. 3.1e-2)
FLAGGED_SEED = {43: 15, 40: 5}


def flagged_case(q):
    """Log mode with a DENSE upstream gradient: weight on states whose posterior is far below 1e-8 (q = 43: the gene
    model, whose codon states are that improbable almost everywhere; q = 40: a dense model with three states that emit
    at 1e-12 only), so the exposed-weight rule flags every sequence."""
    rng = np.random.default_rng([FLAGGED_SEED[q], q])
    b, L = 3, 333
    A, pi = model_of(rng, "gene" if q == 43 else "dense", q)
    E = (rng.random((1, b, L, q)) * 0.9 + 0.05).astype(np.float32)
    if q != 43:
        E[..., 1:, q - 3:] = 1e-12
    G = rng.standard_normal(E.shape).astype(np.float32)
    return dict(A=A[None], pi=pi[None], E=E, G=G)


def floor_decided_case():
    """tests/test_loglik_grad_scan_gpu.py::test_floor_decided_sequence_is_redone with a posterior loss: on the 43-state
    gene model, sequence 1 has a stretch where only one state emits, which the topology leaves after one step."""
    rng = np.random.default_rng(2)
    q, b, L = 43, 3, 900
    A = np.array(gene_model(3)[0])
    pi = np.full(q, 1 / q, dtype=np.float32)
    E = (rng.random((1, b, L, q)) * 0.9 + 0.05).astype(np.float32)
    only = int(np.argmax((A > 0).sum(-1) == 1))              # a state with a single successor
    assert (A[only] > 0).sum() == 1
    E[0, 1, 400:420] = 0.0
    E[0, 1, 400:420, only] = 0.5
    gam = recursions64(A, pi, E[0])[0]
    G = -(gam == gam.max(-1, keepdims=True)).astype(np.float32)[None]
    return dict(A=A[None], pi=pi[None], E=E, G=G)
