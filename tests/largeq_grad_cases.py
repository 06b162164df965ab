"""Inputs and norms of the oracle sweep of the two training entry points above 64 states, on their two evaluations:

  lwalk   hmm_loglik_grad_large, HMM_OPT_GLARGE = 1: the per-sequence walk (csrc/hmm_grad_large.inc: k_gl_walk_fwd,
          k_gl_walk_bwd<64|128>, k_mq_grad_sum, k_mq_grad_pi), q <= 128
  lgemm   hmm_loglik_grad_large, HMM_OPT_GLARGE = 2: per-position GEMMs (k_lq_gemm, k_gl_bpost, k_gl_dA, k_mq_grad_pi)
  pwalk   hmm_posterior_grad_large, HMM_OPT_GLARGE = 1 (csrc/hmm_postgrad_large.inc: k_gl_walk_fwd, k_pgl_walk_rb,
          k_pgl_walk_beta, k_pgl_walk_alpha, k_pg_grad_sum, k_pg_merge, k_pg_sum_rows), q <= 128, both modes
  pgemm   hmm_posterior_grad_large, HMM_OPT_GLARGE = 2 (k_lq_gemm, k_pgl_beta_step, k_pgl_alpha_step, k_gl_dA), both modes

Test infrastructure; imports neither the engine nor a GPU.  tests/test_largeq_grad_sweep_cpu.py proves from the fp64
oracles alone that these inputs can carry the comparison; tests/test_largeq_grad_sweep_gpu.py runs the kernels on them.

A case is a Spec; build(spec) -> dict(A (k,q,q), pi (k,q), E (k,b,L,q), w (k,b) or None, G (k,b,L,q) or None) float32,
deterministic; the inputs depend on (entry point, models, q, b, L, emis, w | G, seed) alone, so the two evaluations of
an entry point and the two modes of the posterior gradient share their arrays.  reference(spec) -> per model the fp64
oracle and the error of its fp32 twin, cached and read-only:
  lwalk, lgemm   oracle.textbook.loglik_grad / loglik in fp64; twin oracle.ref_cell.loglik_grad (fp32 autograd through
                 the restated reference loop on the CPU)                         -- loglik_grad_cases.oracle64 / twin
  pwalk, pgemm   oracle.torch64.posterior_grad in fp64; twin the same function with dtype=torch.float32
                                                                                 -- postgrad_mid_cases.oracle

Tensor norms, exactly those of tests/test_loglik_grad_large_gpu.py and tests/test_posterior_grad_large_gpu.py (each
reported as worst err / tolerance, <= 1 passes; "tensor" as (max|err| - 1e-6) / max|want|, <= 3e-4 passes):
  lwalk, lgemm   dA         present edges (A > 0): 2e-4 max|want|
                 dA/absent  absent edges: |g64(no clamp mask) - g64| + 5e-3 max|want|
                 dpi        2e-4 max|want|
                 dE         2e-5 max|want| + 1e-4 |entry|
                 ll         1e-6 |ll| + 2e-4
  pwalk, pgemm   tensor     max|err| <= 3e-4 max|want| + 1e-6 for each of dA, dpi, dE
Finer norms, as tests/loglik_grad_cases.py and tests/postgrad_mid_cases.py define them, on all four routes:
  dA/row     row i over its present edges / max|want| over those edges, worst i
  dE/seq     max over (t, j) of |err| in sequence s / max|want| in sequence s, worst s
  dE/col     the same per state column j (no chunk-boundary floor vectors here: every route carries it)
with the limit max(FLOOR, 4 e32) per case, model and norm; FLOOR = 2e-4 for the log-likelihood gradients, 3e-4 for the
posterior gradients; e32 the twin's own error under that norm on those very inputs: the factor 4 pays for the
kernel's approximate reciprocals (v_rcp_f32, 1 ulp) and its different summation order.  Nothing in a limit or an
exclusion comes from engine output.

Exclusions, decided from the fp64 reference alone: a row, column or sequence whose reference scale is below SMALL =
1e-30 of the tensor's maximum is held to the tensor norm only.  At most 5 % of a case's rows, columns or sequences may
be excluded, 4 e32 <= 1e-3 in every case and norm, and every clamp a case is meant to engage (E, pi, forward predicted
state, backward predicted state) is active in the fp64 recursion (violations(), asserted by the CPU test).  A case whose
default seed misses a condition takes the first of seed + 10, + 20, ... that meets it (SEEDS).

The three tile-width shapes (b = 3328 or 192) are ordinary cases: their twins run over the whole batch in about a
second each, so they carry every norm over every sequence, the sampled sequences {0, 1, b/2, b - 1} included.
"""
import collections
import functools
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch

import loglik_grad_cases as lc
import postgrad_mid_cases as pm
from largeq_sweep import lq_tile_width

EPS = 1e-16
SMALL_CAP, FINE_FACTOR, FINE_CAP = lc.SMALL_CAP, 4.0, 1e-3
assert (lc.FINE_FLOOR, pm.FINE_FLOOR) == (2e-4, 3e-4) and lc.SMALL == pm.SMALL == 1e-30   # the issue's FLOORs and SMALL
assert (lc.FINE_FACTOR, pm.FINE_FACTOR, lc.FINE_CAP, pm.FINE_CAP) == (FINE_FACTOR, FINE_FACTOR, FINE_CAP, FINE_CAP)
ROUTES = ("lwalk", "lgemm", "pwalk", "pgemm")
GLARGE = {"lwalk": 1, "lgemm": 2, "pwalk": 1, "pgemm": 2}    # HMM_OPT_GLARGE
WALK_MAX = 128                                               # GL_WALK_MAX = GL_Q_WALK: the default route switches above
FINE_NORMS = ("dA/row", "dE/seq", "dE/col")
assert lc.fine_norms("lwalk") == lc.fine_norms("lgemm") == FINE_NORMS and set(pm.FINE_NORMS) == set(FINE_NORMS)

# route: see above.  models: tuple of "dense" | "sparse" (rand_model, primitive) | "tinypi" (sparse, two pi entries
# below eps) | "deadin" (sparse, three states nothing enters, two pi entries below eps) | "gene" (1 + 14 c states) |
# "fclamp" | "bclamp".  emis: "holes" | "blank0" (holes, and the whole first row of each model's heaviest sequence 0) |
# "rare" | "dead" | "clamp" | "mid" (a fifth of the entries 10^U(-16,-6): clamped under eps = 1e-6 only).
# lwalk, lgemm: w = "wide" (+-10^U(-3,3)) | "zeros" (wide, three sequences 0) | "none"; G = "", log = False.
# pwalk, pgemm: G = "dense" (standard normal) | "label" (-(rand < 0.05)); log: POST_LOG?; w = "".
Spec = collections.namedtuple("Spec", "route models q b L emis w G log eps seed")


def kind(spec):
    """"l": hmm_loglik_grad_large, "p": hmm_posterior_grad_large."""
    return spec.route[0]


def spec_id(s):
    what = s.w if kind(s) == "l" else "%s-%s" % (s.G, "log" if s.log else "prob")
    return "%s-%s-q%d-b%d-L%d-%s-%s%s" % (s.route, "+".join(s.models), s.q, s.b, s.L, s.emis, what,
                                          "" if s.eps == EPS else "-eps%g" % s.eps)


def norms(spec):
    return (lc.TENSOR_NORMS if kind(spec) == "l" else ("tensor",)) + FINE_NORMS


def heaviest(c, m):
    """The sequence of model m whose first row "blank0" clears: the largest |w|, or the largest |sum of G| (its weight
    in the log-likelihood term of POST_LOG_NO_LL)."""
    if c["G"] is None:
        return int(np.abs(c["w"][m]).argmax())
    return int(np.abs(c["G"][m].sum((1, 2), dtype=np.float64)).argmax())


def build(spec):
    """Spec -> dict(A, pi, E, w, G) float32 (read-only; w or G None), the same arrays for the same spec in every
    process, for both evaluations of an entry point and for both modes."""
    return _build(spec._replace(route=kind(spec), log=False))


@functools.lru_cache(maxsize=None)
def _build(spec):
    k, q, b, L = len(spec.models), spec.q, spec.b, spec.L
    rng = np.random.default_rng([spec.seed, q, b, L])
    Ms = [lc.build_model(rng, name, q) for name in spec.models]
    A, pi = np.stack([m[0] for m in Ms]), np.stack([m[1] for m in Ms])
    E = lc.draw_E(rng, spec.models, b, L, q, spec.emis)
    w = G = None
    if spec.route == "l":
        w = lc.draw_w(rng, k, b, spec.w)
    elif spec.G == "dense":
        G = rng.standard_normal(E.shape).astype(np.float32)
    elif spec.G == "label":                                  # a cross-entropy against labels
        G = -(rng.random(E.shape) < 0.05).astype(np.float32)
    else:
        raise ValueError(spec.G)
    out = dict(A=A, pi=pi, E=E, w=w, G=G)
    if spec.emis == "blank0":                                # gamma_0 is pi's and R_0's alone, dpi must not lose it
        for m in range(k):
            E[m, heaviest(out, m), 0, :] = 0.0
    for v in out.values():
        if v is not None:
            v.flags.writeable = False
    return out


def reference(spec):
    """-> list over the models of dict(want=(dA, dpi, dE[, ll]) fp64, e32={norm: the fp32 twin's error}, limit={fine
    norm: limit}, small={fine norm: fraction excluded}[, dA_unmasked, dead]); computed once per entry point, inputs
    and mode, read-only."""
    return _reference(spec._replace(route=kind(spec)))


@functools.lru_cache(maxsize=None)
def _reference(spec):
    c = _build(spec._replace(log=False))
    out = []
    for m in range(len(spec.models)):
        A, pi, E = c["A"][m], c["pi"][m], c["E"][m]
        if spec.route == "l":
            w = None if c["w"] is None else c["w"][m]
            out.append(lc.with_twin(lc.oracle64(A, pi, E, w, eps=spec.eps), A, pi, E, w, "lwalk", eps=spec.eps))
        else:
            want = pm.oracle(A, pi, E, c["G"][m], spec.log, eps=spec.eps)
            for x in want:
                x.flags.writeable = False
            e32, small = pm.errors(pm.oracle(A, pi, E, c["G"][m], spec.log, torch.float32, eps=spec.eps), want, A)
            out.append(dict(want=want, e32=e32, small=small,
                            limit={n: max(pm.FINE_FLOOR, pm.FINE_FACTOR * e32[n]) for n in FINE_NORMS}))
    return out


def errors(spec, got, ref_m, A):
    """One model's (dA, dpi, dE[, ll]) against its reference -> ({norm: error}, {fine norm: fraction excluded})."""
    return lc.errors(got, ref_m, A, "lwalk") if kind(spec) == "l" else pm.errors(got, ref_m["want"], A)


def limits(spec, ref_m):
    return lc.limits(ref_m) if kind(spec) == "l" else pm.limits(ref_m)


def post_fine_check(got, A, pi, E, G, log, tag, eps=EPS):
    """lc.fine_check's posterior counterpart, for tests with inputs of their own: (dA, dpi, dE) of one model under the
    finer norms against the fp64 oracle, each at max(3e-4, 4 e32) with e32 measured on these very inputs; prints, then
    asserts."""
    want = pm.oracle(A, pi, E, G, log, eps=eps)
    e32, _ = pm.errors(pm.oracle(A, pi, E, G, log, torch.float32, eps=eps), want, A)
    err, _ = pm.errors(got, want, A)
    lim = {n: max(pm.FINE_FLOOR, pm.FINE_FACTOR * e32[n]) for n in FINE_NORMS}
    for n in FINE_NORMS:
        print("LQGSWEEP %s %s err %.3e limit %.3e e32 %.3e" % (tag, n, err[n], lim[n], e32[n]))
    bad = [(n, err[n], lim[n]) for n in FINE_NORMS if not err[n] <= lim[n]]
    assert not bad, (tag, bad)


def engages(spec):
    """The clamps a case must engage in the fp64 recursion (per model: set of forward / backward / pi / E)."""
    out = []
    for name in spec.models:
        s = set()
        if spec.emis in ("holes", "blank0", "dead", "mid"):
            s.add("E")
        if name in ("tinypi", "deadin"):
            s.add("pi")
        if name == "fclamp":
            s.add("forward")
        if name == "bclamp":
            s |= {"backward", "E"}
        out.append(s)
    return out


def blank0_share(spec, c, m):
    """What dpi loses if the blank first row's sequence drops out of it, over max|dpi| of the reference: the
    log-likelihood gradient's dpi of that sequence alone (for the posterior routes with its weight sum of G, the
    log-likelihood term of POST_LOG_NO_LL)."""
    s = heaviest(c, m)
    wt = c["w"][m, s:s + 1] if c["G"] is None else np.array([c["G"][m, s].sum(dtype=np.float64)])
    alone = lc.textbook.loglik_grad(c["A"][m], c["pi"][m], c["E"][m, s:s + 1], wt, eps=spec.eps)[1]
    return float(np.abs(alone).max())


def violations(spec):
    """The conditions of this module's docstring that `spec` misses, from the references alone ([] = none)."""
    c, bad = build(spec), []
    for m, ref in enumerate(reference(spec)):
        if not all(np.isfinite(x).all() for x in ref["want"]):
            bad.append((m, "not finite"))
        for n in FINE_NORMS:
            if not ref["small"][n] <= SMALL_CAP:
                bad.append((m, n, "small", ref["small"][n]))
            if not FINE_FACTOR * ref["e32"][n] <= FINE_CAP:
                bad.append((m, n, "e32", ref["e32"][n]))
        _, count = pm.forward_backward64(c["A"][m], c["pi"][m], c["E"][m], eps=spec.eps)
        for clamp in engages(spec)[m]:
            if not count[clamp] >= 1:
                bad.append((m, clamp, "not engaged"))
        if spec.emis == "blank0" and kind(spec) == "l":
            if not blank0_share(spec, c, m) > 0.5 * np.abs(ref["want"][1]).max():
                bad.append((m, "blank0 share"))
    return bad


# ---- the cases ----------------------------------------------------------------------------------------------------
WALK_Q2 = (65, 66, 67, 68, 69, 96, 127, 128)                 # two waves, q4 padding, the last active lane
WALK_Q1 = (1, 2, 3, 4, 5, 33, 63, 64)                        # the same entry point, one wave (QB = 64)
GENE_Q = 71                                                  # the five-copy gene model
GEMM_Q = (1, 15, 16, 17, 31, 32, 33, 64, 65, 95, 96, 97, 127, 128, 129, 159, 160, 161, 191, 192, 193, 255, 256, 257)
SWEEP_B, WALK_L, GEMM_L = 3, 41, 9
LENGTHS = (1, 2, 3, 4, 5)                                    # the triple buffer, the ping-pongs, outer = t < L - 2
LENGTH_Q = {90: ROUTES, 130: ("lgemm", "pgemm")}
BATCHES = (1, 4, 5, 15, 16, 17, 63, 64, 65, 130)             # k_gl_dA's groups of 4 at stride 16; the 64-lane strides
BATCH_L = 6
BATCH_Q = {71: (ROUTES, ("gene", "sparse")), 140: (("lgemm", "pgemm"), ("dense", "sparse"))}
TILE_SHAPES = ((192, 1027, 64), (3328, 261, 80), (3328, 344, 96))           # (b, q, tile columns), L = 2
CLAMP_Q = (70, 150)
CLAMP_L = 60
MODES = (False, True)                                        # log?

# Cases whose default seed does not meet the conditions of violations(), with the first seed of seed + 10, + 20, ...
# that does, and why.  All four: one row of the five-copy gene model's dA is 1e-6..1e-7 of the tensor and fp32 autograd
# itself is off there, 4 e32 of dA/row = 3.0e-3 (lwalk, seed 1), 1.1e-3 (pwalk prob, seed 1), 1.4e-3 (b = 65 log, seed 4).
SEEDS = {
    "lwalk-gene-q71-b3-L41-holes-wide": 11, "pwalk-gene-q71-b3-L41-holes-dense-prob": 11,
    "pwalk-gene+sparse-q71-b65-L6-holes-dense-log": 14, "pgemm-gene+sparse-q71-b65-L6-holes-dense-log": 14,
}


def seeded(specs):
    return [s._replace(seed=SEEDS.get(spec_id(s), s.seed)) for s in specs]


def routes_for(q):
    return ROUTES if q <= WALK_MAX else ("lgemm", "pgemm")


def expand(route, models, q, b, L, emis, seed, w="wide", G="dense", eps=EPS, modes=MODES):
    """The Spec of a log-likelihood route, or those of a posterior route in `modes`."""
    if route[0] == "l":
        return [Spec(route, models, q, b, L, emis, w, "", False, eps, seed)]
    return [Spec(route, models, q, b, L, emis, "", G, log, eps, seed) for log in modes]


def walk_state_sweep():
    out = []
    for route in ("lwalk", "pwalk"):
        for n, q in enumerate(WALK_Q2 + WALK_Q1):
            out += expand(route, ("sparse" if n % 2 else "dense",), q, SWEEP_B, WALK_L, "rare" if n % 2 else "holes", 1)
        for emis in ("holes", "rare", "dead"):
            out += expand(route, ("gene",), GENE_Q, SWEEP_B, WALK_L, emis, 1, G="dense" if emis == "holes" else "label")
    return seeded(out)


def gemm_state_sweep():
    out = []
    for route in ("lgemm", "pgemm"):
        for n, q in enumerate(GEMM_Q):
            out += expand(route, ("dense" if n % 2 else "sparse",), q, SWEEP_B, GEMM_L, "holes" if n % 2 else "rare", 1)
    return seeded(out)


def length_sweep():
    return seeded([s for q, routes in LENGTH_Q.items() for route in routes for L in LENGTHS
                   for s in expand(route, ("dense", "sparse"), q, 3, L, "holes", 2)])


def batch_sweep():
    return seeded([s for q, (routes, models) in BATCH_Q.items() for route in routes for b in BATCHES
                   for s in expand(route, models, q, b, BATCH_L, "holes", 4)])


def tile_cases():
    return seeded([s for b, q, _ in TILE_SHAPES for route in ("lgemm", "pgemm")
                   for s in expand(route, ("sparse",), q, b, 2, "holes", 8)])


def weight_cases():
    out = []
    for route, q in (("lwalk", 90), ("lgemm", 90), ("lgemm", 200)):
        out += expand(route, ("dense", "sparse"), q, 65, 7, "holes", 5, w="zeros")
        out += expand(route, ("dense", "sparse"), q, 5, 40, "holes", 5, w="none")
        out += expand(route, ("tinypi", "dense"), q, 5, 40, "holes", 5)
        out += expand(route, ("deadin", "dense"), q, 5, 40, "holes", 5)
        out += expand(route, ("dense", "sparse"), q, 5, 40, "blank0", 5)
    for route in ("pwalk", "pgemm"):
        for G in ("dense", "label"):
            out += expand(route, ("dense", "sparse"), 90, 5, 40, "blank0", 5, G=G)
            out += expand(route, ("tinypi", "dense"), 90, 5, 40, "holes", 5, G=G)
    return seeded(out)


def eps_cases():
    """eps = 1e-6 with emissions between 1e-16 and 1e-6: the clamp is the caller's eps, not the default."""
    return seeded([s for route in ROUTES for s in expand(route, ("dense", "sparse"), 90, 4, 12, "mid", 7, eps=1e-6)])


def clamp_cases():
    out = []
    for q in CLAMP_Q:
        for route in routes_for(q):
            out += expand(route, ("fclamp",), q, 3, CLAMP_L, "clamp", 3)
            if route[0] == "p":
                out += expand(route, ("bclamp",), q, 3, CLAMP_L, "clamp", 3)
    return seeded(out)


def composition_case():
    """autograd.posterior(mode=POST_LOG_NO_LL) above 64 states composes hmm_posterior_grad_large with
    hmm_loglik_grad_large (weights = sum of G per sequence): the inputs of a pwalk blank0 case, the reference
    torch64.posterior_grad(add_loglik=True)."""
    return seeded(expand("pwalk", ("dense",), 80, 5, 40, "blank0", 9, modes=(True,)))[0]


def composition_reference(spec):
    c = build(spec)
    return pm.oracle(c["A"][0], c["pi"][0], c["E"][0], c["G"][0], True, eps=spec.eps, add_loglik=True)


def all_specs():
    return (walk_state_sweep() + gemm_state_sweep() + length_sweep() + batch_sweep() + tile_cases() + weight_cases()
            + eps_cases() + clamp_cases())


def tile_cols(b, q):
    """engine.largeq_tile_cols restated (lq_tile_width of csrc/hmm_largeq.inc, tests/largeq_sweep.py)."""
    return 16 * lq_tile_width(b, q)
