"""Inputs and norms of the oracle sweep of hmm_loglik_grad_walk (65..256 states, the per-sequence walk with the sparse
step, csrc/hmm_gradwq.inc: k_wq_prep, k_gw_fwd, k_gw_bwd, k_gw_sum, k_mq_grad_pi, k_gw_refuse).

Test infrastructure; imports neither the engine nor a GPU, and draws nothing of its own: models, emissions, weights,
oracles and norms are those of tests/loglik_grad_cases.py (build_model, draw_E, draw_w, oracle64, with_twin, errors)
and tests/posterior_walk_cases.py (degree_model).  tests/test_loglik_grad_walk_cpu.py proves from the fp64 oracle and
its fp32 twin alone that these inputs can carry the comparison; tests/test_loglik_grad_walk_gpu.py runs the kernels.

A case is a Spec; build(spec) -> dict(A (k,q,q), pi (k,q), E (k,b,L,q), w (k,b) or None) float32, deterministic and
read-only.  reference(spec) -> per model loglik_grad_cases.with_twin's entry under the route "lwalk" (the fp64 oracle,
the fp32 twin's error e32, the limits of the finer norms), cached and read-only.

Models: "gene" (1 + 14 c states: 71, 127 and 253 are the models of 5, 9 and 18 copies; the intergenic state is the one
hub), "deg0" (exactly 8 predecessors and successors everywhere), "deg1" / "deg2" (7 everywhere and one / two hubs of 9;
deg2 also has two entries of pi below eps), "deg3" (three states above 8: outside the sparse rule, REFUSED).

Norms, the project's own (tests/loglik_grad_cases.py), each reported as err / tolerance or as a relative error:
  dA         present edges (A > 0): 2e-4 max|want|
  dpi        2e-4 max|want|
  dE         2e-5 max|want| + 1e-4 |entry|
  ll         1e-6 |ll| + 2e-4
  dA/row, dE/seq, dE/col   at max(2e-4, 4 e32), route "lwalk"
The dA/absent norm does not apply: hmm_loglik_grad_walk writes exactly 0.0 wherever A == 0, and `off_support` counts
the entries that are not.

Conditions of a case (violations(), asserted by the CPU test): finite references; at most SMALL_CAP = 5 % of rows,
columns or sequences excluded from a finer norm; 4 e32 <= 1e-3; the clamps the case is meant to engage active in the
fp64 recursion.  A case that misses one takes the first of seed + 10, + 20, ... that meets it (SEEDS)."""
import collections
import functools

import numpy as np

import loglik_grad_cases as lc
import postgrad_mid_cases as pm
from loglik_grad_cases import build_model, draw_E, draw_w, errors, oracle64, with_twin
from posterior_walk_cases import degree_model

EPS = 1e-16
Q_MIN, Q_MAX = 65, 256
PF = 8                                                       # WQ_PF: emission rows in flight
ROUTE = "lwalk"
TENSOR_NORMS = ("dA", "dpi", "dE", "ll")
FINE_NORMS = lc.fine_norms(ROUTE)
SMALL_CAP, FINE_FACTOR, FINE_CAP, FINE_FLOOR = lc.SMALL_CAP, lc.FINE_FACTOR, lc.FINE_CAP, lc.FINE_FLOOR
assert FINE_NORMS == ("dA/row", "dE/seq", "dE/col") and (FINE_FLOOR, FINE_FACTOR, FINE_CAP, SMALL_CAP) == (2e-4, 4.0, 1e-3, 0.05)

Spec = collections.namedtuple("Spec", "models q b L emis w eps seed")

GENE_Q = (71, 127, 253)
DEG_Q = (65, 96, 128, 129, 192, 193, 256)                    # one .. four waves, one lane in the last wave, a full one
DEG_KINDS = ("deg0", "deg1", "deg2")
REFUSED = "deg3"
LENGTHS = (1, 2, 3, PF - 1, PF, PF + 1, 2 * PF + 1, 300)
BATCHES = (1, 3, 65, 130)
BATCH_L = 24
EMISSIONS = ("holes", "blank0", "dead", "mid", "rare")
WEIGHTS = ("wide", "zeros", "none")


def spec_id(s):
    return "%s-q%d-b%d-L%d-%s-%s%s" % ("+".join(s.models), s.q, s.b, s.L, s.emis, s.w,
                                       "" if s.eps == EPS else "-eps%g" % s.eps)


def model(rng, kind, q):
    """-> A (q,q), pi (q,) float32."""
    if kind == "gene":
        return build_model(rng, "gene", q)
    hubs = int(kind[3:])
    A = degree_model(rng, q, hubs)
    pi = rng.random(q) + 0.1
    if hubs == 2:
        pi[rng.choice(q, 2, replace=False)] = 1e-20
    return A, (pi / pi.sum()).astype(np.float32)


def build(spec):
    return _build(spec._replace(eps=EPS))                    # eps does not enter the draw


@functools.lru_cache(maxsize=None)
def _build(spec):
    k, q, b, L = len(spec.models), spec.q, spec.b, spec.L
    rng = np.random.default_rng([spec.seed, q, b, L])
    Ms = [model(rng, name, q) for name in spec.models]
    A, pi = np.stack([np.array(m[0]) for m in Ms]), np.stack([np.array(m[1]) for m in Ms])
    E = draw_E(rng, spec.models, b, L, q, spec.emis)
    w = draw_w(rng, k, b, spec.w)
    if spec.emis == "blank0":                                # the whole first row of each model's heaviest sequence
        E[np.arange(k), np.abs(w).argmax(-1), 0, :] = 0.0
    out = dict(A=A, pi=pi, E=E, w=w)
    for v in out.values():
        if v is not None:
            v.flags.writeable = False
    return out


@functools.lru_cache(maxsize=None)
def reference(spec):
    """-> list over the models of dict(want=(dA, dpi, dE, ll) fp64, e32, limit, small, dead), read-only; None for a
    refused model."""
    c = build(spec)
    out = []
    for m, name in enumerate(spec.models):
        if name == REFUSED:
            out.append(None)
            continue
        A, pi, E, w = c["A"][m], c["pi"][m], c["E"][m], None if c["w"] is None else c["w"][m]
        out.append(with_twin(oracle64(A, pi, E, w, unmasked=False, eps=spec.eps), A, pi, E, w, ROUTE, eps=spec.eps))
    return out


def check(got, ref_m, A):
    """(dA, dpi, dE, ll) of one model -> ({norm: error}, {norm: limit}, off_support): the tensor norms as err /
    tolerance (limit 1), the finer norms as relative errors (limit max(2e-4, 4 e32)), and how many entries of dA with
    A == 0 are not exactly 0.0."""
    dA, dpi, dE, ll = (np.asarray(x, np.float64) for x in got)
    wA, wpi, wE, wll = ref_m["want"]
    present = np.asarray(A) > 0
    e, _ = errors(got, ref_m, A, ROUTE, tensor=False)
    e["dA"] = lc._worst(np.abs(dA - wA)[present], 2e-4 * np.abs(wA).max())
    e["dpi"] = lc._worst(np.abs(dpi - wpi), 2e-4 * np.abs(wpi).max())
    e["dE"] = lc._worst(np.abs(dE - wE), 2e-5 * np.abs(wE).max() + 1e-4 * np.abs(wE))
    e["ll"] = lc._worst(np.abs(ll - wll), 1e-6 * np.abs(wll) + 2e-4)
    limit = dict({n: 1.0 for n in TENSOR_NORMS}, **ref_m["limit"])
    off = int(np.count_nonzero(np.asarray(got[0])[np.asarray(A) == 0]))
    return e, limit, off


def engages(spec):
    """The clamps a case must engage in the fp64 recursion (per model: set of forward / pi / E)."""
    out = []
    for name in spec.models:
        s = set()
        if spec.emis in ("holes", "blank0", "dead") or (spec.emis == "mid" and spec.eps > EPS):
            s.add("E")
        if name == "deg2":
            s.add("pi")
        if name == "gene" and spec.emis == "dead" and spec.eps > EPS:
            s.add("forward")                                 # (see eps_cases: not reachable at eps = 1e-16)
        out.append(s)
    return out


def violations(spec):
    """The conditions of this module's docstring that `spec` misses, from the references alone ([] = none)."""
    c, bad = build(spec), []
    for m, ref in enumerate(reference(spec)):
        if ref is None:
            continue
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
    return bad


# ---- the cases ----------------------------------------------------------------------------------------------------
# Cases whose default seed does not meet the conditions of violations(), with the first seed of seed + 10, + 20, ...
# that does.
# The five-copy model at L = 300: one column of dE at 4 e32 = 1.1e-3 (seed 1).  The eps = 1e-6 case of 71 states: 4 e32
# of dA/row and dE/col = 6.5e-3 / 4.0e-3 (seed 7), 2.1e-3 / 2.2e-2 (17), 1.8e-2 / 5.6e-3 (27) — with a fifth of the
# emissions between 1e-16 and 1e-6 the fp32 twin crosses the clamp at other entries than the fp64 recursion.
SEEDS = {"gene-q71-b3-L300-holes-wide": 11, "gene+deg1-q71-b4-L12-mid-wide-eps1e-06": 37}


def seeded(specs):
    return [s._replace(seed=SEEDS.get(spec_id(s), s.seed)) for s in specs]


def gene_sweep():
    """The three gene models, long enough for the normalisers to matter, under the three emission patterns of the
    gene sweeps of tests/largeq_grad_cases.py."""
    return seeded([Spec(("gene",), q, 3, 300 if emis == "holes" else 41, emis, "wide", EPS, 1)
                   for q in GENE_Q for emis in ("holes", "rare", "dead")])


def state_sweep():
    out = []
    for n, q in enumerate(DEG_Q):
        for i, kind in enumerate(DEG_KINDS):
            out.append(Spec((kind,), q, 3, 2 * PF + 1, ("holes", "rare", "mid")[(n + i) % 3], "wide", EPS, 1))
    return seeded(out)


def length_sweep():
    return seeded([Spec(models, q, 3, L, "holes", "wide", EPS, 2)
                   for q, models in ((71, ("gene", "deg1")), (193, ("deg2", "deg0"))) for L in LENGTHS])


def batch_sweep():
    return seeded([Spec(("gene", "deg2") if b < 130 else ("gene",), 127, b, BATCH_L, "holes", "wide", EPS, 4)
                   for b in BATCHES])


def weight_cases():
    m = ("gene", "deg1")
    return seeded([Spec(m, 127, 65, PF - 1, "holes", "zeros", EPS, 5), Spec(m, 127, 5, 40, "holes", "none", EPS, 5),
                   Spec(m, 127, 5, 40, "blank0", "wide", EPS, 5), Spec(("deg0", "deg2"), 256, 5, 40, "blank0", "wide", EPS, 5)])


def eps_cases():
    """eps = 1e-6 with emissions between 1e-16 and 1e-6: the clamp is the caller's eps, not the default.  The shapes are
    those whose fp32 twin stays under the cap: at 253 states the gene model's twin missed it with every seed of 7 .. 77
    (4 e32 of dA/row >= 2e-2), the one-hub degree model meets it; the "dead" gene case with L = 41 at 127 states
    missed it likewise, L = 9 at 71 states meets it.  That last case is the one that engages the FORWARD clamp of the
    predicted state on a gene model: under eps = 1e-16 no "dead" gene case reaches it in the fp64 recursion (seeds
    1 .. 71 at 71, 127 and 253 states) — every state of the gene topology keeps a predecessor that the pattern never
    zeroes —, so those cases are held to the E clamp alone, as in tests/loglik_grad_cases.py."""
    return seeded([Spec(("gene", "deg1"), 71, 4, 12, "mid", "wide", 1e-6, 7),
                   Spec(("deg1",), 253, 4, 12, "mid", "wide", 1e-6, 7),
                   Spec(("gene",), 71, 3, PF + 1, "dead", "wide", 1e-6, 7)])


def refused_case():
    """A refused model next to a served one in one call."""
    return seeded([Spec((REFUSED, "deg1"), 96, 3, 2 * PF + 1, "holes", "wide", EPS, 6)])[0]


def all_specs():
    return gene_sweep() + state_sweep() + length_sweep() + batch_sweep() + weight_cases() + eps_cases()
