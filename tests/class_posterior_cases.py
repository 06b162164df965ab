"""Inputs, norms and routing predictions of the oracle sweep of hmm_class_posterior / hmm_class_posterior_grad (1..16
states: class posteriors P_c[t] = the sum of gamma_t over the states of class c, and the gradient of a loss on P or
log P; csrc/hmm_class_posterior.inc, the ClassOut policy of csrc/hmm_engine.hip and the PgClassG loader of
csrc/hmm_postgrad.inc / hmm_postgrad_chunked.inc).

Test infrastructure; imports neither the engine nor a GPU.  Models, emission patterns, forced chunk lengths and clamp
constructions are those of tests/postgrad_small_cases.py (`ps`, imported, not copied): a case's A, pi and E are
ps.build(state_spec(case)).  Added here: a class table (table_of) and the upstream gradient Gc (k,b,L,C), "dense"
(standard normal), "label" (-1 at the class with the largest fp64 posterior of every position, 0 elsewhere: a
cross-entropy against class labels) or "labelx" (the same with -0.5 on every empty class as well).  Tables: "gene" = posterior_decode_mid_cases.gene_classes (6 classes), "id" =
range(q), "one" = a single class, "r2" / "r5" / "r16" = random_map with that many classes (C > q leaves the classes
from q on empty), "empty" = five classes of which class 2 has no state.

Oracle: tests/class_posterior_walk_cases.py's (oracle.torch64.posterior in fp64, P = gamma @ one-hot(table), log P where
Gc != 0, autograd; an empty class passes nothing), which is the state-level oracle with the gradient expanded to the
states; its fp32 twin is the same code in float32.  Norms and limits are postgrad_small_cases': tensor 3e-4 + 1e-6; the
fine norms dE/col, dE/seq, dA/row at max(3e-4, 4 e32 of the fp32 twin); q = 1 (and the table "one", where P is
identically 1 and the true gradient identically 0) are held to an absolute bound, max(1e-6, 4 x the twin's largest
entry) per tensor, as ps holds q = 1.

routing(spec): what the device-side rules must decide per sequence, from the fp64 recursion alone: ps.routing's F64 and
primitivity, and in log mode the CLASS form of the exposed-weight rule,
  exposed = (F64 sum_{P_c >= 1e-8} |Gc| / P_c + sum_{P_c < 1e-8} |Gc|) / sum |Gc|   (threshold 1e-4),
with the verdicts "chunk" / "whole" / "open" as in ps (a factor 4 either side).

A class whose states all have posterior exactly 0 in fp32 has no place in an fp64 table (the fp64 posterior is 1e-47,
not 0, and fp64 autograd divides by it): tests/test_class_posterior_gpu.py builds that case itself and compares the
engine with itself.

Conditions of a case (violations(), asserted by tests/test_class_posterior_cpu.py): finite oracle; at most one, or 5 %,
of the rows, columns or sequences excluded from a finer norm (rows of A without a present edge not counted:
tests/test_postgrad_small_cpu.py's rule); 4 e32 <= 1e-3 under the fine norms it is held to; in log mode the fp64
P_c >= MIN_P = 1e-6 wherever Gc != 0 on a non-empty class; the clamps the case is meant to engage active."""
import collections
import functools

import numpy as np
import torch

import class_posterior_walk_cases as cw
import posterior_decode_mid_cases as dm
import postgrad_mid_cases as pm
import postgrad_small_cases as ps

EPS = ps.EPS
MIN_P = cw.MIN_P
SMALL_CAP = cw.SMALL_CAP
MAX_STATES, MAX_CLASSES = 16, 16
EMPTY_CLASS = 2
FINE_NORMS, FINE_FLOOR, FINE_FACTOR, FINE_CAP = ps.FINE_NORMS, ps.FINE_FLOOR, ps.FINE_FACTOR, ps.FINE_CAP
TENSOR_REL, TENSOR_ABS = ps.TENSOR_REL, ps.TENSOR_ABS
assert (TENSOR_REL, TENSOR_ABS, FINE_FLOOR, FINE_FACTOR) == (3e-4, 1e-6, 3e-4, 4.0)

Spec = collections.namedtuple("Spec", "models q b L emis G log seed T table eps")


def spec_id(s):
    return "%s-q%d-b%d-L%d-%s-%s-%s-%s%s%s" % ("+".join(s.models), s.q, s.b, s.L, s.emis, s.G, s.table,
                                                "log" if s.log else "prob", "-T%d" % s.T if s.T else "",
                                                "" if s.eps == EPS else "-eps%g" % s.eps)


def state_spec(s):
    """The case of tests/postgrad_small_cases.py whose A, pi and E this case runs on."""
    return ps.Spec(s.models, s.q, s.b, s.L, s.emis, "dense", s.log, s.seed, s.T)


def table_of(spec):
    return _table(spec.table, spec.q)


@functools.lru_cache(maxsize=None)
def _table(kind, q):
    rng = np.random.default_rng([91, q, len(kind)])
    if kind == "gene":
        assert q == 15
        return tuple(dm.gene_classes(q)), 6
    if kind == "id":
        return tuple(range(q)), q
    if kind == "one":
        return (0,) * q, 1
    if kind == "empty":
        return tuple(dm.random_map(rng, q, 5, empty=(EMPTY_CLASS,))), 5
    C = {"r2": 2, "r5": 5, "r16": 16}[kind]
    return tuple(dm.random_map(rng, q, C)), C


def build(spec):
    """Spec -> dict(A, pi, E, G (k,b,L,C)) float32 (read-only), the same arrays for the same spec in every process."""
    return _build(spec._replace(eps=EPS) if spec.G == "dense" else spec)


@functools.lru_cache(maxsize=None)
def _build(spec):
    c = ps.build(state_spec(spec))
    table, C = table_of(spec)
    k, b, L = len(spec.models), spec.b, spec.L
    rng = np.random.default_rng([spec.seed, spec.q, b, L, C, 17])
    if spec.G == "dense":
        G = rng.standard_normal((k, b, L, C)).astype(np.float32)
    elif spec.G in ("label", "labelx"):
        G = np.empty((k, b, L, C), np.float32)
        empty = np.bincount(np.asarray(table), minlength=C) == 0
        for m in range(k):
            P = pm.forward_backward64(c["A"][m], c["pi"][m], c["E"][m], eps=spec.eps)[0] @ cw.one_hot(table, C)
            G[m] = -(P.argmax(-1)[..., None] == np.arange(C)).astype(np.float32)
            if spec.G == "labelx":
                G[m][..., empty] = -0.5
    else:
        raise ValueError(spec.G)
    out = dict(A=c["A"], pi=c["pi"], E=c["E"], G=G)
    G.flags.writeable = False
    return out


def expand(Gc, table):
    return cw.expand(Gc, table)


def zero_truth(spec):
    """The true gradient is identically 0: one state, or one class (P = 1 whatever the parameters)."""
    return spec.q == 1 or spec.table == "one"


@functools.lru_cache(maxsize=None)
def reference(spec):
    """-> list over the models of dict(want=(dA, dpi, dE) fp64, P (b,L,C) fp64, e32, limit, small, norms, absolute)."""
    c = build(spec)
    table, C = table_of(spec)
    out = []
    for m, name in enumerate(spec.models):
        A, pi, E, G = c["A"][m], c["pi"][m], c["E"][m], c["G"][m]
        full = cw.oracle(A, pi, E, G, table, C, spec.log, eps=spec.eps)
        want, P = full[:3], full[3]
        for x in full:
            x.flags.writeable = False
        twin = cw.oracle(A, pi, E, G, table, C, spec.log, torch.float32, eps=spec.eps)[:3]
        e32, small = ps.errors(twin, want, A, False, ps.floor_columns(name, A))
        del e32["dA/absent"]
        limit = {n: max(FINE_FLOOR, FINE_FACTOR * e32[n]) for n in FINE_NORMS}
        absolute = [max(ps.Q1_ABS, FINE_FACTOR * float(np.abs(x).max())) for x in twin] if zero_truth(spec) else None
        norms = FINE_NORMS if (all(np.isfinite(x).all() for x in twin) and not zero_truth(spec)) else ()
        out.append(dict(want=want, P=P, e32=e32, limit=limit, small=small, absolute=absolute, norms=norms))
    return out


def check(got, ref_m, A, name, per_chunk):
    """(dA, dpi, dE) of one model -> ({norm: error}, {norm: limit}) over the norms the case is held to."""
    e, _ = ps.errors(tuple(np.asarray(x, np.float64) for x in got), ref_m["want"], A, per_chunk, ps.floor_columns(name, A))
    lim = {n: ref_m["limit"][n] for n in ref_m["norms"]}
    if ref_m["absolute"] is None:
        lim["tensor"] = TENSOR_REL
    if per_chunk:
        lim["dA/absent"] = ps.ABSENT_REL
    return {n: e[n] for n in lim}, lim


@functools.lru_cache(maxsize=None)
def routing(spec):
    c = build(spec)
    table, C = table_of(spec)
    M = cw.one_hot(table, C)
    out = []
    for m in range(len(spec.models)):
        gam, count, ah, Rb = pm.forward_backward64(c["A"][m], c["pi"][m], c["E"][m], eps=spec.eps, parts=True)
        F = spec.eps * (1.0 / (ah * Rb).sum(-1)).sum(-1)
        ratio = F / ps.EXACT_DELTA
        exposed = None
        if spec.log:
            P = gam @ M
            w = np.abs(c["G"][m].astype(np.float64))
            tiny = P < ps.PG_TINY_GAMMA
            gp = np.where(tiny, 0.0, w / np.where(tiny, 1.0, P)).sum((1, 2))
            exposed = (F * gp + np.where(tiny, w, 0.0).sum((1, 2))) / np.maximum(w.sum((1, 2)), 1e-300)
            ratio = np.maximum(ratio, exposed / ps.PC_LOG_EXPOSED)
        prim = ps.primitive(c["A"][m], spec.eps)
        verdict = ["whole" if (not prim or r >= ps.MARGIN) else "chunk" if r <= 1 / ps.MARGIN else "open" for r in ratio]
        out.append(dict(F=F, exposed=exposed, primitive=prim, verdict=verdict, count=count))
    return out


def shipped_per_chunk(spec):
    return ps.shipped_per_chunk(state_spec(spec))


def serial_bounds(spec):
    """(fewest, most) sequences the whole-sequence sweeps serve under the shipped routing."""
    n = len(spec.models) * spec.b
    if not shipped_per_chunk(spec):
        return n, n
    v = [x for r in routing(spec) for x in r["verdict"]]
    return v.count("whole"), n - v.count("chunk")


def forced_per_chunk(spec):
    """The cases the GPU test also runs under HMM_OPT_PGCHUNK = 2 (no certificate): ps.forced_per_chunk's rule."""
    r = routing(spec)
    return (spec.q > 1 and ps.chunks(state_spec(spec)) >= 2 and all(x["primitive"] for x in r)
            and all(x["count"]["forward"] == 0 and x["count"]["backward"] == 0 for x in r))


def engages(spec):
    out = ps.engages(state_spec(spec))
    if spec.eps != EPS and spec.emis == "rare":
        for s in out:
            s.add("E")                                       # 1e-10 lies below the caller's eps
    return out


def violations(spec):
    c, bad = build(spec), []
    table, C = table_of(spec)
    used = np.bincount(np.asarray(table), minlength=C) > 0
    for m, ref in enumerate(reference(spec)):
        if not all(np.isfinite(x).all() for x in ref["want"]):
            bad.append((m, "not finite"))
        empty_rows = int((~(c["A"][m] > 0).any(-1)).sum())
        for n in ref["norms"]:
            among = spec.q if n != "dE/seq" else spec.b
            exempt = ref["small"][n] * among - (empty_rows if n == "dA/row" else 0)
            if not exempt <= max(1, SMALL_CAP * among) + 1e-9:
                bad.append((m, n, "small", ref["small"][n]))
            if not FINE_FACTOR * ref["e32"][n] <= FINE_CAP:
                bad.append((m, n, "e32", ref["e32"][n]))
        if ref["absolute"] is not None and not max(ref["absolute"]) <= ps.Q1_OF_G * float(np.abs(c["G"][m]).max()):
            bad.append((m, "absolute", ref["absolute"]))
        if spec.log:
            on = (c["G"][m] != 0) & used
            if on.any() and not ref["P"][on].min() >= MIN_P:
                bad.append((m, "min P", float(ref["P"][on].min())))
        count = routing(spec)[m]["count"]
        for clamp in engages(spec)[m]:
            if not count[clamp] >= 1:
                bad.append((m, clamp, "not engaged"))
    return bad


# ---- the cases ----------------------------------------------------------------------------------------------------
MODES = (False, True)
STATES = (1, 2, 7, 15, 16)
LENGTHS = (1, 2, 3, 15, 16, 17, 33)
BATCHES = (1, 3, 5, 130)
# Cases whose default seed does not meet the conditions of violations(), with the first seed of seed + 10, + 20, ...
# that does: 4 e32 of dA/row = 2.0e-3 (the gene model at L = 15, log mode); the as-shipped model, whose columns at 1e-4
# of the tensor carry an e32 of 2.5e-2 under dE/col (tests/postgrad_small_cases.py has the same case at seeds 27 / 37);
# a pi entry of 1e-20 on a state nothing enters (ps.SEEDS' first group).
SEEDS = {"gene+dense-q15-b2-L15-holes-label-r5-log": 12, "gene+shipped-q15-b3-L100-plain-dense-gene-prob-T16": 27,
         "dense-d-q15-b3-L100-holes-label-r5-log": 11}


def seeded(specs):
    return [s._replace(seed=SEEDS.get(spec_id(s), s.seed)) for s in specs]


def grad_kind(log):
    """Log mode with a dense Gc weighs log P of classes below MIN_P: the cross-entropy's gradient there."""
    return "label" if log else "dense"


def S(models, q, b, L, emis, G, log, seed, T, table, eps=EPS):
    return Spec(tuple(models), q, b, L, emis, G, log, seed, T, table, eps)


def state_sweep():
    """Every q of the table on the engine's own chunk length (L = 100: several chunks), every kind of table."""
    out = []
    for log in MODES:
        g = grad_kind(log)
        out += [S(("dense",), 1, 3, 100, "holes", "dense", log, 1, 0, "one"),
                S(("dense",), 2, 3, 100, "holes", g, log, 1, 0, "r16"),            # C > q
                S(("sparse",), 2, 3, 100, "plain", "dense", log, 1, 0, "r2"),
                S(("simple7",), 7, 3, 100, "holes", g, log, 1, 0, "r5"),
                S(("dense",), 7, 3, 100, "holes", g, log, 1, 0, "id"),
                S(("gene",), 15, 3, 100, "holes", g, log, 1, 0, "gene"),
                S(("dense",), 16, 3, 100, "holes", g, log, 1, 0, "id"),            # the table range(q), 16 classes
                S(("sparse",), 16, 3, 100, "holes", g, log, 1, 0, "r16"),
                S(("dense",), 15, 3, 100, "plain", "dense", log, 1, 0, "one"),     # all states in one class
                S(("gene",), 15, 3, 100, "plain", "labelx" if log else "dense", log, 1, 0, "empty")]    # Gc on an empty class
    return seeded(out)


def length_sweep():
    return seeded([S(("gene", "dense"), 15, 2, L, "holes", grad_kind(log), log, 2, 0, "r5") for log in MODES
                   for L in LENGTHS])


def geometry_sweep():
    """Forced chunk lengths 16 and 48 (and the engine's own) at L = 100 and 300."""
    return seeded([S((name,), q, 2, L, "plain", grad_kind(log), log, 5, T, table) for log in MODES
                   for name, q, table in (("gene", 15, "gene"), ("dense", 7, "r2"))
                   for T, L in ((16, 33), (16, 100), (48, 100), (48, 300), (0, 300))])


def batch_sweep():
    """Five chunks per sequence: b = 1, 3, 5, 130 give 5, 15, 25, 650 chunks, ragged rows of four chunks per wave."""
    return seeded([S(("dense", "sparse") if b < 130 else ("dense",), 7, b, 65, "plain", grad_kind(log), log, 4, 16, "r5")
                   for log in MODES for b in BATCHES])


def emission_cases():
    out = []
    for log in MODES:
        for name, q, table in (("gene", 15, "gene"), ("simple7", 7, "r2")):
            out.append(S((name,), q, 3, 100, "rare", "label", log, 1, 16, table))
            out.append(S((name,), q, 3, 100, "dead", "label", log, 1, 16, table))
        out.append(S(("gene",), 15, 3, 203, "stretch", grad_kind(log), log, 3, 16, "gene"))
        out += [S((kind,), q, 3, 130, "clamp", "dense", log, 3, 16, "r2") for q in (7, 16)
                for kind in ("fclamp", "fclamp2", "bclamp")]
    return seeded(out)


def model_cases():
    """Reducible and non-primitive models (routed per model), and two different models in one call."""
    out = []
    for log in MODES:
        g = grad_kind(log)
        out += [S(("dense", "triu"), 7, 3, 100, "plain", g, log, 6, 16, "r2"),
                S(("sparse-d",), 16, 3, 100, "holes", g, log, 1, 16, "r5"),
                S(("dense-d",), 15, 3, 100, "holes", g, log, 1, 0, "r5"),
                S(("gene", "shipped"), 15, 3, 100, "plain", g, log, 7, 16, "gene")]
    return seeded(out)


def eps_cases():
    """eps = 1e-6 with emissions of 1e-10: the clamp is the caller's eps, not the default."""
    return seeded([S(("gene",), 15, 3, 100, "rare", "label", log, 7, 16, "gene", eps=1e-6) for log in MODES]
                  + [S(("dense",), 7, 3, 33, "rare", "label", log, 7, 0, "r5", eps=1e-6) for log in MODES])


def all_specs():
    return (state_sweep() + length_sweep() + geometry_sweep() + batch_sweep() + emission_cases() + model_cases()
            + eps_cases())
