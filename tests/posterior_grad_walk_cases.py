"""Inputs and norms of the oracle sweep of hmm_posterior_grad_walk (65..256 states, the per-sequence walk with the
sparse step, csrc/hmm_postgradwq.inc: k_wq_prep, k_gw_fwd, k_pgw_rb, k_pgw_beta, k_pgw_alpha, k_pgw_sum, k_pg_sum_rows,
k_gw_refuse).

Test infrastructure; imports neither the engine nor a GPU, and draws nothing of its own: models are those of
tests/loglik_grad_walk_cases.py (model: gene 71 / 127 / 253, deg0 / deg1 / deg2, the refused deg3), emissions those of
tests/loglik_grad_cases.py (draw_E), the upstream gradient G is drawn as tests/largeq_grad_cases.py draws it ("dense":
standard normal, "label": -(rand < 0.05)), the oracle is tests/postgrad_mid_cases.py's (oracle: oracle.torch64.
posterior_grad by autograd in fp64, with its fp32 twin).  tests/test_posterior_grad_walk_cpu.py proves from the
references alone that these inputs can carry the comparison; tests/test_posterior_grad_walk_gpu.py runs the kernels.

A case is a Spec; build(spec) -> dict(A (k,q,q), pi (k,q), E (k,b,L,q), G (k,b,L,q)) float32, deterministic and
read-only, the same arrays in both modes.  reference(spec) -> per model dict(want, e32, limit, small), cached and
read-only; None for a refused model.

Norms, the project's own (tests/postgrad_mid_cases.py: errors, limits):
  tensor                   max|err| <= 3e-4 max|want| + 1e-6 for each of dA, dpi, dE
  dA/row, dE/seq, dE/col   at max(3e-4, 4 e32), e32 the fp32 twin's error under that norm on these inputs
One adaptation: hmm_posterior_grad_walk defines dA on the support of A, so the reference dA — the oracle's and its
twin's — is multiplied by (A > 0) before any norm, and `off_support` counts the entries of the engine's dA with A == 0
that are not exactly 0.0; that count must be 0.

Conditions of a case (violations(), asserted by the CPU test), decided from the references alone: finite oracle and
twin; at most SMALL_CAP = 5 % of rows, columns or sequences excluded from a finer norm; 4 e32 <= 1e-3; the clamps the
case is meant to engage active in postgrad_mid_cases.forward_backward64.  A case that misses one takes the first of
seed + 10, + 20, ... that meets it (SEEDS)."""
import collections
import functools

import numpy as np
import torch

import loglik_grad_cases as lc
import loglik_grad_walk_cases as wc
import postgrad_mid_cases as pm

EPS = 1e-16
Q_MIN, Q_MAX = 65, 256
REFUSED = wc.REFUSED
NORMS = ("tensor", "dA/row", "dE/seq", "dE/col")
FINE_NORMS = NORMS[1:]
SMALL_CAP, FINE_FACTOR, FINE_CAP, FINE_FLOOR = lc.SMALL_CAP, pm.FINE_FACTOR, pm.FINE_CAP, pm.FINE_FLOOR
assert set(pm.FINE_NORMS) == set(FINE_NORMS) and (FINE_FLOOR, FINE_FACTOR, FINE_CAP, SMALL_CAP) == (3e-4, 4.0, 1e-3, 0.05)
assert (pm.TENSOR_REL, pm.TENSOR_ABS) == (3e-4, 1e-6)

# G: "dense" | "label"; log: POST_LOG?
Spec = collections.namedtuple("Spec", "models q b L emis G log eps seed")

GENE_Q = (71, 127, 253)
DEG_Q = (65, 96, 128, 129, 192, 193, 256)                    # one .. four waves, one lane in the last wave, a full one
DEG_KINDS = ("deg0", "deg1", "deg2")
LENGTHS = (1, 2, 3, 7, 8, 9, 17, 300)                        # around the ring depths; the position-0 and successor branches
BATCHES = (1, 3, 65, 130)
BATCH_L = 24
MODES = (False, True)


def spec_id(s):
    return "%s-q%d-b%d-L%d-%s-%s-%s%s" % ("+".join(s.models), s.q, s.b, s.L, s.emis, s.G, "log" if s.log else "prob",
                                          "" if s.eps == EPS else "-eps%g" % s.eps)


def build(spec):
    return _build(spec._replace(eps=EPS, log=False))         # neither eps nor the mode enters the draw


@functools.lru_cache(maxsize=None)
def _build(spec):
    q, b, L = spec.q, spec.b, spec.L
    rng = np.random.default_rng([spec.seed, q, b, L])
    Ms = [wc.model(rng, name, q) for name in spec.models]
    A, pi = np.stack([np.array(m[0]) for m in Ms]), np.stack([np.array(m[1]) for m in Ms])
    E = lc.draw_E(rng, spec.models, b, L, q, spec.emis)
    if spec.G == "dense":
        G = rng.standard_normal(E.shape).astype(np.float32)
    elif spec.G == "label":                                  # a cross-entropy against labels
        G = -(rng.random(E.shape) < 0.05).astype(np.float32)
    else:
        raise ValueError(spec.G)
    out = dict(A=A, pi=pi, E=E, G=G)
    for v in out.values():
        v.flags.writeable = False
    return out


def on_support(grads, A):
    """(dA, dpi, dE) with dA multiplied by (A > 0)."""
    return (np.asarray(grads[0], np.float64) * (np.asarray(A) > 0),) + tuple(grads[1:])


@functools.lru_cache(maxsize=None)
def reference(spec):
    """-> list over the models of dict(want=(dA on the support, dpi, dE) fp64, e32, limit, small), read-only; None for
    a refused model."""
    c = build(spec)
    out = []
    for m, name in enumerate(spec.models):
        if name == REFUSED:
            out.append(None)
            continue
        A, pi, E, G = c["A"][m], c["pi"][m], c["E"][m], c["G"][m]
        want = on_support(pm.oracle(A, pi, E, G, spec.log, eps=spec.eps), A)
        for x in want:
            x.flags.writeable = False
        e32, small = pm.errors(on_support(pm.oracle(A, pi, E, G, spec.log, torch.float32, eps=spec.eps), A), want, A)
        out.append(dict(want=want, e32=e32, small=small,
                        limit={n: max(FINE_FLOOR, FINE_FACTOR * e32[n]) for n in FINE_NORMS}))
    return out


def check(got, ref_m, A):
    """(dA, dpi, dE) of one model -> ({norm: error}, {norm: limit}, off_support): how many entries of dA with A == 0
    are not exactly 0.0."""
    e, _ = pm.errors(tuple(np.asarray(x, np.float64) for x in got), ref_m["want"], A)
    off = int(np.count_nonzero(np.asarray(got[0])[np.asarray(A) == 0]))
    return e, pm.limits(ref_m), off


def engages(spec):
    """The clamps a case must engage in the fp64 recursion (per model: set of forward / backward / pi / E)."""
    out = []
    for name in spec.models:
        s = set()
        if spec.emis in ("holes", "dead") or (spec.emis == "mid" and spec.eps > EPS):
            s.add("E")
        if name == "deg2":
            s.add("pi")
        if name == "gene" and spec.emis in ("holes", "rare") and spec.eps == EPS and spec.L >= 41:
            s |= {"forward", "backward"}                     # the gene sweep: hundreds of times each
        if name == "gene" and spec.emis == "dead" and spec.eps > EPS:
            s.add("forward")
        out.append(s)
    return out


def violations(spec):
    """The conditions of this module's docstring that `spec` misses, from the references alone ([] = none)."""
    c, bad = build(spec), []
    for m, ref in enumerate(reference(spec)):
        if ref is None:
            continue
        if not all(np.isfinite(x).all() for x in ref["want"]) or not all(np.isfinite(v) for v in ref["e32"].values()):
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
# that does (SEED_NOTES: what the default seed missed).
# All three are the 18-copy gene model: 4 e32 of dA/row = 3.7e-3 in prob mode under "holes" (seed 1; 1.03e-3 at seed 11)
# and 1.4e-3 under "dead" (seed 1); under "rare" with label G in log mode the references of seed 1 are not finite.
SEEDS = {"gene-q253-b3-L120-holes-dense-prob": 21, "gene-q253-b3-L41-dead-dense-prob": 11,
         "gene-q253-b3-L41-rare-label-log": 11}


def seeded(specs):
    return [s._replace(seed=SEEDS.get(spec_id(s), s.seed)) for s in specs]


def both(models, q, b, L, emis, G, seed, eps=EPS):
    return [Spec(models, q, b, L, emis, G, log, eps, seed) for log in MODES]


def gene_sweep():
    out = []
    for q in GENE_Q:
        out += both(("gene",), q, 3, 120, "holes", "dense", 1)
        out += both(("gene",), q, 3, 41, "rare", "label", 1)
        out += both(("gene",), q, 3, 41, "dead", "dense", 1)
    return seeded(out)


def state_sweep():
    out = []
    for n, q in enumerate(DEG_Q):
        for i, kind in enumerate(DEG_KINDS):
            out += both((kind,), q, 3, 17, ("holes", "rare", "mid")[(n + i) % 3], ("dense", "label")[(n + i) % 2], 1)
    return seeded(out)


def length_sweep():
    return seeded([s for q, models in ((71, ("gene", "deg1")), (193, ("deg2", "deg0"))) for L in LENGTHS
                   for s in both(models, q, 3, L, "holes", "dense", 2)])


def batch_sweep():
    return seeded([s for b in BATCHES
                   for s in both(("gene", "deg2") if b < 130 else ("gene",), 127, b, BATCH_L, "holes", "dense", 4)])


def eps_cases():
    """eps = 1e-6 with emissions between 1e-16 and 1e-6: the clamp is the caller's eps, not the default.  The "dead"
    gene case engages the forward clamp of the predicted state on a gene model."""
    return seeded(both(("gene", "deg1"), 71, 4, 12, "mid", "dense", 7, eps=1e-6)
                  + both(("deg1",), 253, 4, 12, "mid", "dense", 7, eps=1e-6)
                  + both(("gene",), 71, 3, 9, "dead", "dense", 7, eps=1e-6))


def refused_cases():
    """A refused model next to a served one in one call, both modes."""
    return seeded(both((REFUSED, "deg1"), 96, 3, 17, "holes", "dense", 6))


def all_specs():
    return gene_sweep() + state_sweep() + length_sweep() + batch_sweep() + eps_cases()
