"""Inputs, references and limits of the sweep of the caller-chosen clamp eps through the forward / backward / posterior
/ decode / posterior-gradient entry points for 1..64 states (tests/test_eps_sweep_cpu.py, tests/test_eps_sweep_gpu.py).

Test infrastructure; imports neither the engine nor a GPU.  The model builders, the gradient oracle and the gradient
norms are those of tests/postgrad_mid_cases.py and tests/postgrad_small_cases.py (imported, not copied).

A case is a Spec(models, q, b, L, emis, eps, T, seed):
  models  a tuple of names, one per model of the call:
          "gene"     the compiled gene topologies: 7 states (params.edges_simple), 15 (params.intended_A15), 29 / 43 /
                     57 (the 2- / 3- / 4-copy transitioner, which take the sparse step of the one-wave walk);
          "gene-fd"  the 15-state model under HMM_OPT_FORCE_DENSE (the dense MFMA reduce);
          "dense"    a random dense model (every entry of A >= 4e-3: no mixture clamp below eps = 1e-3);
          "triu"     an upper-triangular model: its support is reducible, k_topo_check routes the model;
          "thin"     tests/postgrad_mid_cases.forward_clamp_model with the edge 0 -> D at sqrt(1e-16 eps): in the support
                     (A > eps) at the default eps and outside it at the case's, so the model's route changes with eps;
                     D emits with probability 1, so its floor mass shows in gamma.
  emis    "plain"    U(0.05, 0.95);
          "rare"     a fifth of the entries 10^U(-16, log10 eps + 2): on both sides of the case's eps, all above 1e-16;
          "zeros"    10 % exact zeros, state 0 kept alive;
          "blank"    one all-zero row and two consecutive ones (with L = 1: the row): the denormal-range mark of the
                     reduces;
          "edge"     "rare", and a tenth of the entries exactly float32(eps) or one of its two fp32 neighbours: pins the
                     strict comparison E > eps of the gradients.
  eps     the caller's value; the oracle and the engine both see float(np.float32(eps)) (eps32), so that `> eps` is the
          same comparison on both sides.  CONTROL = 1e-16 is the control of every case.
  T       HMM_OPT_CHUNK for the call (0: the engine's own rule).

Three tables: posterior_cases() (hmm_posterior in its three modes, hmm_forward, hmm_backward, and with the identity
map hmm_posterior_decode / _mid), refusal_cases() (eps below HMM_EPS_MIN = 1e-18: 1e-20 and 1e-30 with blank rows; the
kernels' arithmetic needs eps^2 to be a normal fp32 number, include/hmm_engine.h) and grad_cases() (hmm_posterior_grad
in both modes, hmm_posterior_grad_scan).

HANDOVER and handover_case(q) are the inputs of what the sweep found: the reverse cell's clamp active at the last
position of a chunk alone, where the vector comes from the chunk scan (16-state rows, 32-lane and 64-lane rows).

Tolerances (tests/test_engine_gpu.py, unchanged): gamma 2e-5, log-likelihood 1e-6 |ll| + 2e-4, log alpha / log beta
through assert_log_close_in_probability_space.  e32 is the error of the same recursion run in fp32 numpy against fp64;
a case that misses a tolerance on the device is conditioning only if 4 e32 exceeds it (CONDITIONED below names such
cases; the limit is then max(tolerance, 4 e32)).

e32 of the posterior cases (tests/test_eps_sweep_cpu.py prints every case's): gamma and log-likelihood / tolerance
  gene-q15-b3-L200-plain-eps1e-06-T16          2.5e-07  0.00
  gene-q15-b3-L200-plain-eps0.001-T16          2.8e-07  0.00
  gene-q15-b3-L200-rare-eps1e-10-T16           1.8e-07  0.00
  gene-q15-b3-L200-zeros-eps1e-06-T16          2.4e-07  0.00
  gene-q15-b2-L641-blank-eps1e-06-T16          3.8e-07  0.00
  gene-q15-b3-L200-edge-eps1e-06-T16           2.8e-07  0.00
  gene-q15-b2-L1-blank-eps1e-10-T16            3.5e-09  0.00
  gene-q15-b5-L17-rare-eps0.001-T16            2.3e-07  0.00
  gene-q15-b2-L641-rare-eps1e-10               2.2e-07  0.01
  gene-q7-b3-L200-rare-eps1e-06-T16            2.0e-07  0.01
  gene-q7-b4-L17-zeros-eps0.001-T16            1.3e-07  0.00
  gene-q7-b2-L641-blank-eps1e-10-T16           2.5e-07  0.00
  gene-q7-b2-L641-blank-eps1e-06-T16           3.0e-07  0.00
  gene-q7-b2-L961-blank-eps1e-06-T16           2.7e-07  0.00
  gene-fd-q15-b3-L200-rare-eps1e-06-T16        2.4e-07  0.00
  gene-fd-q15-b2-L641-blank-eps0.001-T16       4.7e-07  0.00
  dense-q1-b5-L17-rare-eps1e-06-T16            0.0e+00  0.00
  dense-q2-b3-L200-rare-eps1e-06-T16           9.3e-08  0.00
  dense-q5-b3-L200-rare-eps0.001-T16           1.1e-07  0.00
  dense-q5-b2-L1-blank-eps1e-06-T16            1.3e-08  0.00
  dense-q13-b3-L200-edge-eps0.001-T16          1.0e-07  0.00
  dense-q16-b2-L641-rare-eps0.001-T16          7.0e-08  0.00
  dense-q16-b2-L641-blank-eps1e-06-T16         5.6e-08  0.01
  dense-q13-b2-L641-blank-eps1e-10-T16         8.7e-08  0.00
  triu-q7-b3-L200-rare-eps0.001-T16            1.2e-07  0.00
  thin-q7-b3-L200-plain-eps0.001-T16           1.2e-07  0.00
  thin-q16-b2-L200-plain-eps0.001-T16          5.2e-08  0.00
  dense+triu-q7-b2-L200-rare-eps0.001-T16      1.8e-07  0.00
  gene-q29-b3-L641-rare-eps1e-10-T16           2.7e-07  0.00
  gene-q29-b3-L203-plain-eps1e-06              2.3e-07  0.00
  gene-q29-b2-L641-blank-eps1e-06-T16          3.6e-07  0.00
  gene-q29-b4-L17-zeros-eps0.001-T16           1.8e-07  0.00
  gene-q43-b2-L641-rare-eps1e-06-T16           2.4e-07  0.00
  gene-q43-b3-L17-edge-eps1e-06-T16            1.1e-07  0.00
  gene-q57-b3-L100-zeros-eps1e-06-T16          1.8e-07  0.00
  gene-q57-b1-L641-blank-eps1e-10-T16          1.6e-07  0.00
  dense-q17-b3-L200-rare-eps0.001-T16          7.6e-08  0.00
  dense-q32-b2-L641-rare-eps0.001-T16          4.3e-08  0.00
  dense-q33-b2-L641-rare-eps0.001-T16          3.5e-08  0.00
  dense-q48-b3-L100-blank-eps1e-06-T16         1.8e-08  0.00
  dense-q64-b5-L17-rare-eps0.001-T16           1.8e-08  0.00
  dense-q64-b1-L641-zeros-eps0.001-T16         1.3e-08  0.00
  dense-q64-b2-L1-blank-eps1e-06-T16           3.7e-09  0.00
  triu-q20-b2-L641-rare-eps0.001-T16           1.3e-07  0.00
  thin-q24-b2-L641-plain-eps0.001-T16          4.3e-08  0.00
  dense+triu-q20-b2-L641-rare-eps0.001-T16     1.5e-07  0.00
  gene-q15-b3-L200-blank-eps1e-20-T16          3.4e-07  0.01
  gene-q15-b2-L17-blank-eps1e-30-T16           1.8e-07  0.00
  dense-q5-b2-L641-blank-eps1e-30-T16          1.4e-07  0.00
  gene-q29-b2-L641-blank-eps1e-20-T16          2.5e-07  0.00
  dense-q48-b3-L100-blank-eps1e-30-T16         1.8e-08  0.00

e32 of the gradient cases, per norm (tensor, dE/col, dE/seq, dA/row; the chunk / whole variants of a case share one
reference):
  gene-q15-b3-L200-rare-eps1e-06-T16           prob 4.7e-07  2.7e-05  4.7e-07  5.5e-06
  gene-q15-b3-L200-rare-eps1e-06-T16           log  3.3e-07  2.0e-07  1.2e-07  9.4e-06
  gene-q15-b3-L200-edge-eps1e-10-T16           prob 4.2e-07  1.5e-04  4.5e-07  3.3e-06
  gene-q15-b3-L200-edge-eps1e-10-T16           log  4.6e-07  1.9e-07  1.8e-07  2.9e-06
  dense-q5-b3-L200-edge-eps0.001-T16           prob 5.8e-07  1.1e-07  1.5e-07  9.9e-07
  dense-q5-b3-L200-edge-eps0.001-T16           log  6.0e-07  1.8e-07  1.8e-07  6.1e-07
  gene-q7-b3-L100-zeros-eps1e-06-T16           prob 1.7e-06  5.6e-05  6.9e-06  1.1e-06
  gene-q7-b3-L100-zeros-eps1e-06-T16           log  1.2e-06  1.1e-06  4.9e-07  1.1e-06
  dense-q16-b3-L203-edge-eps0.001-T16          prob 2.7e-07  2.7e-07  1.7e-07  7.8e-07
  dense-q16-b3-L203-edge-eps0.001-T16          log  3.9e-07  1.9e-07  1.6e-07  6.1e-07
  thin-q7-b3-L200-plain-eps0.001-T16           prob 4.9e-07  5.2e-07  2.0e-07  5.7e-07
  thin-q7-b3-L200-plain-eps0.001-T16           log  4.1e-07  1.4e-07  1.5e-07  8.0e-07
  dense-q2-b3-L17-edge-eps1e-06-T16            prob 6.8e-07  1.6e-07  1.6e-07  1.5e-06
  dense-q2-b3-L17-edge-eps1e-06-T16            log  1.9e-06  1.2e-07  2.0e-07  1.9e-06
  gene-q29-b3-L203-rare-eps1e-06               prob 9.2e-07  9.2e-05  5.5e-06  5.8e-05
  gene-q29-b3-L203-rare-eps1e-06               log  4.2e-07  2.1e-07  1.1e-07  6.4e-06
  dense-q33-b3-L100-edge-eps0.001              prob 1.9e-07  3.6e-07  2.6e-07  8.0e-07
  dense-q33-b3-L100-edge-eps0.001              log  4.4e-07  2.0e-07  1.7e-07  7.4e-07
  gene-q57-b2-L60-edge-eps1e-06                prob 4.7e-07  4.3e-05  1.3e-06  7.0e-05
  gene-q57-b2-L60-edge-eps1e-06                log  1.5e-06  1.9e-07  1.9e-07  3.3e-06
  dense-q64-b2-L50-rare-eps0.001               prob 0.0e+00  4.6e-07  3.1e-07  5.6e-07
  dense-q64-b2-L50-rare-eps0.001               log  3.6e-07  2.3e-07  1.5e-07  4.4e-07
  gene-q29-b2-L641-edge-eps1e-06-T16           prob 5.5e-07  1.1e-05  4.9e-07  1.7e-05
  gene-q29-b2-L641-edge-eps1e-06-T16           log  7.1e-07  7.1e-07  7.1e-07  6.5e-06
  gene-q43-b2-L641-rare-eps1e-06-T16           prob 1.0e-06  4.2e-05  1.0e-06  2.3e-05
  gene-q43-b2-L641-rare-eps1e-06-T16           log  1.1e-06  1.9e-07  1.9e-07  6.7e-06
"""
import collections
import functools
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch

import postgrad_mid_cases as pm
from oracle import params, textbook

CONTROL = 1e-16
EPS_MIN, EPS_MAX = 1e-18, 1e-3                               # include/hmm_engine.h: HMM_EPS_MIN, HMM_EPS_MAX
TOL_GAMMA = 2e-5
DISCRIMINATING = 10.0                                        # a case moves by this many tolerances against the control
GENE_COPIES = {29: 2, 43: 3, 57: 4}

Spec = collections.namedtuple("Spec", "models q b L emis eps T seed")

# cases whose limit on the device is max(tolerance, 4 e32): {spec_id: {output: e32}} (module docstring)
CONDITIONED = {}


def spec_id(s):
    return "%s-q%d-b%d-L%d-%s-eps%g%s" % ("+".join(s.models), s.q, s.b, s.L, s.emis, s.eps, "-T%d" % s.T if s.T else "")


def eps32(eps):
    return float(np.float32(eps))


def tol_loglik(ll64):
    return 1e-6 * np.abs(ll64) + 2e-4


def thin_edge(eps):
    return float(np.sqrt(CONTROL * eps))


@functools.lru_cache(maxsize=None)
def gene_small(q):
    if q == 15:
        A = params.intended_A15().numpy().astype(np.float32)
    else:
        ed = params.edges_simple()
        logits = params.init_logits(ed, 1)
        A = params.dense_A(ed, np.where(logits == 0, 1e-30, logits), 7).numpy().astype(np.float32)
    pi = np.full(q, 1.0 / q, dtype=np.float32)
    A.flags.writeable = pi.flags.writeable = False
    return A, pi


def build_model(rng, name, q, eps):
    if name in ("gene", "gene-fd"):
        return gene_small(q) if q <= 16 else pm.gene_model(GENE_COPIES[q])
    if name == "dense":
        return pm.rand_model(rng, q)
    if name == "triu":
        A, pi = pm.rand_model(rng, q)
        A = np.triu(A).astype(np.float64)
        return (A / A.sum(-1, keepdims=True)).astype(np.float32), pi
    if name == "thin":
        return pm.forward_clamp_model(rng, q, edge=thin_edge(eps))
    raise ValueError(name)


def build(spec):
    """Spec -> dict(A (k,q,q), pi (k,q), E (k,b,L,q)) float32, read-only, the same arrays in every process."""
    return _build(spec)


@functools.lru_cache(maxsize=None)
def _build(spec):
    k, q, b, L = len(spec.models), spec.q, spec.b, spec.L
    rng = np.random.default_rng([spec.seed, q, b, L, int(round(-np.log10(spec.eps)))])
    Ms = [build_model(rng, name, q, spec.eps) for name in spec.models]
    A, pi = np.stack([m[0] for m in Ms]), np.stack([m[1] for m in Ms])
    E = (rng.random((k, b, L, q)) * 0.9 + 0.05).astype(np.float32)
    e32 = np.float32(spec.eps)
    if spec.emis == "plain":
        pass
    elif spec.emis in ("rare", "edge"):
        rare = rng.random(E.shape) < 0.2
        E[rare] = (10.0 ** rng.uniform(-16.0, np.log10(spec.eps) + 2.0, int(rare.sum()))).astype(np.float32)
        if spec.emis == "edge":
            at = rng.random(E.shape) < 0.1
            trio = np.array([np.nextafter(e32, np.float32(0)), e32, np.nextafter(e32, np.float32(1))], np.float32)
            E[at] = trio[rng.integers(0, 3, int(at.sum()))]
    elif spec.emis == "zeros":
        dead = rng.random(E.shape) < 0.1
        dead[..., 0] = False
        E[dead] = 0.0
    elif spec.emis == "blank":
        if L == 1:
            E[:] = 0.0
        else:
            one, two = L // 3, min(2 * L // 3, L - 2)
            E[..., one, :] = 0.0
            E[..., two:two + 2, :] = 0.0
    else:
        raise ValueError(spec.emis)
    for m, name in enumerate(spec.models):
        if name == "thin":
            E[m, ..., q - 1] = 1.0
    out = dict(A=A, pi=pi, E=E)
    for v in out.values():
        v.flags.writeable = False
    return out


# ---- references ---------------------------------------------------------------------------------------------------
def recursion32(A, pi, E, eps):
    """oracle/textbook.py's recursions (forward, backward, posterior) with every array and operation in fp32, but for
    the running sums of the normalisers' fp32 logs, which are fp64 as in the kernels (include/hmm_engine.h) ->
    gamma, loglik, log alpha, log beta: what rounding alone costs."""
    f = np.float32
    A, pi, E, eps = np.asarray(A, f), np.asarray(pi, f), np.asarray(E, f), f(eps)
    b, L, q = E.shape
    Ec = np.maximum(E, eps)
    ah, Rb = np.empty((b, L, q), f), np.empty((b, L, q), f)
    ll, sc = np.empty((b, L)), np.empty((b, L))
    state, acc = np.broadcast_to(pi, (b, q)), np.zeros(b)
    for t in range(L):
        sf = Ec[:, t] * np.maximum(state if t == 0 else state @ A, eps)
        S = sf.sum(-1, keepdims=True, dtype=f)
        acc = acc + np.log(S[:, 0])
        state = sf / S
        ah[:, t], ll[:, t] = state, acc
    state, acc = np.ones((b, q), f), np.zeros(b)
    for t in range(L - 1, -1, -1):
        R = np.maximum(state if t == L - 1 else state @ A.T, eps)
        Rb[:, t], sc[:, t] = R, acc
        sf = Ec[:, t] * R
        S = sf.sum(-1, keepdims=True, dtype=f)
        acc = acc + np.log(S[:, 0])
        state = sf / S
    g = ah * Rb
    with np.errstate(divide="ignore"):
        return g / g.sum(-1, keepdims=True, dtype=f), ll[:, -1], np.log(ah) + ll[..., None], np.log(Rb) + sc[..., None]


def oracle64(A, pi, E, eps):
    """One model -> dict(gamma, ll, la, lb) of oracle/textbook.py at eps32(eps)."""
    e = eps32(eps)
    gamma, ll = textbook.posterior(A, pi, E, eps=e)
    la, _ = textbook.log_alpha(A, pi, E, eps=e)
    return dict(gamma=gamma, ll=ll, la=la, lb=textbook.log_beta(A, E, eps=e))


@functools.lru_cache(maxsize=None)
def reference(spec):
    """-> list over the models of dict(gamma, ll, la, lb: fp64 at the case's eps; control: the same at CONTROL;
    e32: {"gamma": max |gamma32 - gamma64|, "ll": max |ll32 - ll64| / tol_loglik}); computed once, read-only."""
    c = build(spec)
    out = []
    for m in range(len(spec.models)):
        r = oracle64(c["A"][m], c["pi"][m], c["E"][m], spec.eps)
        r["control"] = oracle64(c["A"][m], c["pi"][m], c["E"][m], CONTROL)
        g32, ll32, _, _ = recursion32(c["A"][m], c["pi"][m], c["E"][m], spec.eps)
        r["e32"] = dict(gamma=float(np.abs(g32 - r["gamma"]).max()),
                        ll=float((np.abs(ll32 - r["ll"]) / tol_loglik(r["ll"])).max()))
        for v in (r["gamma"], r["ll"], r["la"], r["lb"]):
            v.flags.writeable = False
        out.append(r)
    return out


def moved(spec):
    """How far the fp64 oracle moves between CONTROL and the case's eps, in tolerances: the worst model's
    (gamma, loglik)."""
    g = ll = 0.0
    for r in reference(spec):
        g = max(g, float(np.abs(r["gamma"] - r["control"]["gamma"]).max()) / TOL_GAMMA)
        ll = max(ll, float((np.abs(r["ll"] - r["control"]["ll"]) / tol_loglik(r["ll"])).max()))
    return g, ll


def limit(spec, output):
    """The factor on the stated tolerance of `output` ("gamma" | "ll") for the case: 1 unless CONDITIONED names it."""
    e32 = CONDITIONED.get(spec_id(spec), {}).get(output)
    if e32 is None:
        return 1.0
    return max(1.0, 4.0 * e32 / (TOL_GAMMA if output == "gamma" else 1.0))


# ---- the posterior family -----------------------------------------------------------------------------------------
def P(models, q, b, L, emis, eps, T=16, seed=1):
    return Spec((models,) if isinstance(models, str) else tuple(models), q, b, L, emis, eps, T, seed)


HANDOVER = P("gene", 7, 2, 961, "blank", 1e-6)
HANDOVER_AT = (1, 223)                                       # sequence, position: the last one of chunk 13 at T = 16


def backward_clamps(A, pi, E, eps):
    """The positions (sequence, t) at which the reverse cell's clamp max(A bh, eps) is active in the fp64 recursion."""
    A, E = np.asarray(A, np.float64), np.maximum(np.asarray(E, np.float64), eps)
    b, L, q = E.shape
    out, R = [], np.ones((b, q))
    for t in range(L - 1, 0, -1):
        sb = E[:, t] * R
        raw = (sb / sb.sum(-1, keepdims=True)) @ A.T
        out += [(int(s), t - 1) for s in np.where((raw <= eps).any(-1))[0]]
        R = np.maximum(raw, eps)
    return sorted(out)


HANDOVER_Q = (12, 24, 48)                                    # 16-state rows, 32-lane rows, 64-lane rows
HANDOVER_EPS, HANDOVER_T, HANDOVER_L, HANDOVER_POS = 1e-3, 16, 641, 16 * 20 - 1


@functools.lru_cache(maxsize=None)
def handover_case(q):
    """One sequence of a dense model whose state q - 1 has the single successor q - 2, which all but cannot emit the
    first observation of chunk 20: the reverse cell's clamp is active at HANDOVER_POS alone, the last position of chunk
    19, where state q - 1 is lifted from 1e-12 of the others to eps = 1e-3.  No forward clamp, no other reverse clamp
    (tests/test_eps_sweep_cpu.py) -> dict(A (1,q,q), pi (1,q), E (1,1,L,q)), read-only."""
    rng = np.random.default_rng([1, q, HANDOVER_L])
    A, pi = pm.rand_model(rng, q)
    A = A.copy()
    A[q - 1] = 0.0
    A[q - 1, q - 2] = 1.0
    E = (rng.random((1, 1, HANDOVER_L, q)) * 0.9 + 0.05).astype(np.float32)
    E[0, 0, HANDOVER_POS + 1, q - 2] = 1e-12
    out = dict(A=A[None], pi=pi[None], E=E)
    for v in out.values():
        v.flags.writeable = False
    return out


def small_cases():
    """1..16 states.  T = 16: 200 positions are 13 chunks (windows with their margin fit), 641 are 41 (the two-level
    scan of more than 32 chunks)."""
    return [
        P("gene", 15, 3, 200, "plain", 1e-6), P("gene", 15, 3, 200, "plain", 1e-3),
        P("gene", 15, 3, 200, "rare", 1e-10), P("gene", 15, 3, 200, "zeros", 1e-6),
        P("gene", 15, 2, 641, "blank", 1e-6), P("gene", 15, 3, 200, "edge", 1e-6),
        P("gene", 15, 2, 1, "blank", 1e-10), P("gene", 15, 5, 17, "rare", 1e-3),
        P("gene", 15, 2, 641, "rare", 1e-10, T=0),
        P("gene", 7, 3, 200, "rare", 1e-6), P("gene", 7, 4, 17, "zeros", 1e-3), P("gene", 7, 2, 641, "blank", 1e-10),
        # windows.  HANDOVER (L = 961): in its second sequence the reverse cell's clamp is active at position 223 alone,
        # the last one of chunk 13, where the vector comes from the chunk scan: the certificate has to weigh it there
        P("gene", 7, 2, 641, "blank", 1e-6), HANDOVER,
        P("gene-fd", 15, 3, 200, "rare", 1e-6), P("gene-fd", 15, 2, 641, "blank", 1e-3),
        P("dense", 1, 5, 17, "rare", 1e-6), P("dense", 2, 3, 200, "rare", 1e-6), P("dense", 5, 3, 200, "rare", 1e-3),
        P("dense", 5, 2, 1, "blank", 1e-6), P("dense", 13, 3, 200, "edge", 1e-3), P("dense", 16, 2, 641, "rare", 1e-3),
        P("dense", 16, 2, 641, "blank", 1e-6), P("dense", 13, 2, 641, "blank", 1e-10),
        P("triu", 7, 3, 200, "rare", 1e-3), P("thin", 7, 3, 200, "plain", 1e-3), P("thin", 16, 2, 200, "plain", 1e-3),
        P(("dense", "triu"), 7, 2, 200, "rare", 1e-3),
    ]


def mid_cases():
    """17..64 states: 17..32 always plan the chunked scan (32-lane rows), 33..64 for few long sequences (64-lane rows);
    the rest is the one-wave walk."""
    return [
        P("gene", 29, 3, 641, "rare", 1e-10), P("gene", 29, 3, 203, "plain", 1e-6, T=0),
        P("gene", 29, 2, 641, "blank", 1e-6), P("gene", 29, 4, 17, "zeros", 1e-3),
        P("gene", 43, 2, 641, "rare", 1e-6), P("gene", 43, 3, 17, "edge", 1e-6),
        P("gene", 57, 3, 100, "zeros", 1e-6), P("gene", 57, 1, 641, "blank", 1e-10),
        P("dense", 17, 3, 200, "rare", 1e-3), P("dense", 32, 2, 641, "rare", 1e-3),
        P("dense", 33, 2, 641, "rare", 1e-3), P("dense", 48, 3, 100, "blank", 1e-6),
        P("dense", 64, 5, 17, "rare", 1e-3), P("dense", 64, 1, 641, "zeros", 1e-3), P("dense", 64, 2, 1, "blank", 1e-6),
        P("triu", 20, 2, 641, "rare", 1e-3), P("thin", 24, 2, 641, "plain", 1e-3),
        P(("dense", "triu"), 20, 2, 641, "rare", 1e-3),
    ]


def posterior_cases():
    return small_cases() + mid_cases()


def refusal_cases():
    """eps below HMM_EPS_MIN: every entry point refuses the call (HMM_ERR_BAD_ARGUMENT).  The inputs are kept, with the
    blank rows that make them discriminating, so that the cases can be served again should the domain grow."""
    return [P("gene", 15, 3, 200, "blank", 1e-20), P("gene", 15, 2, 17, "blank", 1e-30),
            P("dense", 5, 2, 641, "blank", 1e-30), P("gene", 29, 2, 641, "blank", 1e-20),
            P("dense", 48, 3, 100, "blank", 1e-30)]


def is_mid(spec):
    return spec.q > 16


# ---- decoding -----------------------------------------------------------------------------------------------------
def class_map(spec):
    """(table, C, n_max) of the class-map decode of a case: the gene classes for 15 states, five round-robin classes
    otherwise (one class for q = 1, q classes below 5 states)."""
    import posterior_decode_ref as ref
    if spec.q == 15:
        return list(ref.GENE_CLASSES), 5, ref.GENE_NMAX
    C = min(5, spec.q)
    table = [s % C for s in range(spec.q)]
    return table, C, max(table.count(c) for c in range(C))


def decode_cases():
    """The cases posterior_decode runs with a class map (the identity map runs on every posterior case): those whose
    oracle margin clears the rule on 99 % of the positions (the dense 64-state case with zeros does on 98 %: left out)."""
    return [s for s in posterior_cases() if s.L >= 100 and (s.emis in ("rare", "edge")
                                                            or (s.emis == "zeros" and s.models[0] == "gene"))]


def decode_margin_rule(n_max):
    """tests/test_posterior_decode_gpu.py: labels are compared where the oracle's margin between its two best classes
    exceeds 2 n_max 2e-5."""
    return 2 * n_max * TOL_GAMMA


# ---- the posterior gradients --------------------------------------------------------------------------------------
GSpec = collections.namedtuple("GSpec", "spec log route")     # route: "chunk" (PGCHUNK 1) | "whole" (PGCHUNK 0) | "scan"


def gspec_id(g):
    return "%s-%s-%s" % (spec_id(g.spec), "log" if g.log else "prob", g.route)


def grad_cases():
    small = [P("gene", 15, 3, 200, "rare", 1e-6), P("gene", 15, 3, 200, "edge", 1e-10),
             P("dense", 5, 3, 200, "edge", 1e-3), P("gene", 7, 3, 100, "zeros", 1e-6),
             P("dense", 16, 3, 203, "edge", 1e-3), P("thin", 7, 3, 200, "plain", 1e-3),
             P("dense", 2, 3, 17, "edge", 1e-6)]
    mid = [P("gene", 29, 3, 203, "rare", 1e-6, T=0), P("dense", 33, 3, 100, "edge", 1e-3, T=0),
           P("gene", 57, 2, 60, "edge", 1e-6, T=0), P("dense", 64, 2, 50, "rare", 1e-3, T=0)]
    # (seed 3: with seeds 1 and 2 one column of dE is 1e-4 of its tensor and 4 e32 of dE/col passes the cap of 1e-3)
    scan = [P("gene", 29, 2, 641, "edge", 1e-6, seed=3), P("gene", 43, 2, 641, "rare", 1e-6)]
    return ([GSpec(s, log, route) for s in small for log in (False, True) for route in ("chunk", "whole")]
            + [GSpec(s, log, "whole") for s in mid for log in (False, True)]
            + [GSpec(s, log, "scan") for s in scan for log in (False, True)])


def grad_input(g):
    """The upstream gradient of a case: dense standard normal, seeded."""
    s = g.spec
    rng = np.random.default_rng([s.seed, s.q, s.b, s.L, 77])
    G = rng.standard_normal((len(s.models), s.b, s.L, s.q)).astype(np.float32)
    G.flags.writeable = False
    return G


@functools.lru_cache(maxsize=None)
def grad_reference(g):
    """-> list over the models of dict(want=(dA, dpi, dE) fp64 at the case's eps, control=the same at CONTROL,
    e32={norm: fp32 twin's error}, limit={norm: limit}): the norms and limits of tests/postgrad_mid_cases.py."""
    c, G, e = build(g.spec), grad_input(g), eps32(g.spec.eps)
    out = []
    for m in range(len(g.spec.models)):
        # torch.maximum splits the gradient at a tie E == eps; the kernels' convention is the clamped side (dE = 0
        # wherever E <= eps, include/hmm_engine.h).  The oracle sees the tie entries one fp32 ulp lower: max(E, eps) and
        # with it every value is unchanged, and the subgradient is the clamped side's.
        E = np.where(c["E"][m] == np.float32(e), np.nextafter(np.float32(e), np.float32(0)), c["E"][m])
        args = (c["A"][m], c["pi"][m], E, G[m], g.log)
        want = pm.oracle(*args, eps=e)
        twin = pm.oracle(*args, dtype=torch.float32, eps=e)
        control = pm.oracle(*args, eps=CONTROL)
        e32, _ = pm.errors(twin, want, c["A"][m])
        lim = {n: max(pm.FINE_FLOOR, pm.FINE_FACTOR * e32[n]) for n in pm.FINE_NORMS}
        lim["tensor"] = pm.TENSOR_REL
        out.append(dict(want=want, control=control, e32=e32, limit=lim))
    return out


def grad_moved(g):
    """The worst tensor's max |want - control| / (3e-4 max |want|): how far the gradient moves with eps, in limits."""
    worst = 0.0
    for r in grad_reference(g):
        for w, c in zip(r["want"], r["control"]):
            top = float(np.abs(w).max())
            if top > 0:
                worst = max(worst, float(np.abs(w - c).max()) / (pm.TENSOR_REL * top))
    return worst
