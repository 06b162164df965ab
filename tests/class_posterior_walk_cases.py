"""Inputs and norms of the oracle sweep of hmm_class_posterior_walk / hmm_class_posterior_grad_walk (65..256 states:
class posteriors P_c[t] = the sum of gamma_t over the states of class c, and the gradient of a loss on P or log P;
csrc/hmm_wideq.inc: ClassWide, csrc/hmm_postgradwq.inc: k_pgw_beta_class, k_pgw_alpha_class, k_pgw_class_quot).

Test infrastructure; imports neither the engine nor a GPU.  Models are those of tests/loglik_grad_walk_cases.py (model:
gene 71 / 127 / 253, deg0 / deg1 / deg2, the refused deg3), emissions those of tests/loglik_grad_cases.py (draw_E), as
tests/posterior_grad_walk_cases.py draws them.  Class tables (table_of): "gene" = posterior_decode_mid_cases.
gene_classes (6 classes), "r2" / "r5" / "r16" = random_map with that many classes, "empty" = five classes of which
class 2 has no state, "one" = a single class.  The upstream gradient Gc (k,b,L,C) is "dense" (standard normal) or
"label" (-1 at one random non-empty class per position, 0 elsewhere: a cross-entropy against class labels).

Oracle (oracle): oracle.torch64.posterior in fp64, P = gamma @ one-hot(table), log P where Gc != 0, loss = sum Gc P or
sum Gc log P, autograd.  An empty class passes nothing (the header's definition: G' = 0 where P_c == 0), so Gc is
multiplied by (class not empty) before the loss.  Its fp32 twin is the same code with dtype=float32.

Norms, limits and errors are tests/postgrad_mid_cases.py's four:
  tensor                   max|err| <= 3e-4 max|want| + 1e-6 for each of dA, dpi, dE
  dA/row, dE/seq, dE/col   at max(3e-4, 4 e32), e32 the fp32 twin's error under that norm on these inputs
with the adaptation of tests/posterior_grad_walk_cases.py: the reference dA is multiplied by (A > 0), and the engine's dA
must hold exact zeros wherever A == 0 (off_support).  For the table "one" P is identically 1, the true gradient is
identically 0 and what the oracle returns is its own rounding noise (1e-17 .. 1e-14): a relative norm has no scale
there (any fp32 error is 1e9 of that noise, so no seed could meet 4 e32 <= 1e-3), and such a case is held to the tensor
norm alone, unchanged — in effect its absolute part, 1e-6 — on the condition that the fp32 twin itself meets it.  The
five-copy gene model does not (its twin's dpi is off by 9.6e-6, its dA by 6.1e-6, and seeds 18 .. 48 miss it as
seed 8 does: fp32 does not cancel those terms to 1e-6), so the single-class cases are those of a degree model whose
twin does (at most 2.7e-7).

Conditions of a case (violations(), asserted by the CPU test), decided from the references alone: finite oracle and
twin; at most SMALL_CAP = 5 % of rows, columns or sequences excluded from a finer norm; 4 e32 <= 1e-3; in log mode the
fp64 P_c >= MIN_P = 1e-6 wherever Gc != 0 (on non-empty classes); for the table "one" the twin within the tensor norm; the clamps the case is meant to engage active in
postgrad_mid_cases.forward_backward64.  A case that misses one takes the first of seed + 10, + 20, ... that meets it
(SEEDS)."""
import collections
import functools

import numpy as np
import torch

import loglik_grad_cases as lc
import loglik_grad_walk_cases as wc
import posterior_decode_mid_cases as dm
import posterior_grad_walk_cases as pc
import postgrad_mid_cases as pm
from oracle import torch64

EPS = 1e-16
Q_MIN, Q_MAX = 65, 256
MAX_CLASSES = 16
MIN_P = 1e-6
REFUSED = wc.REFUSED
NORMS = ("tensor", "dA/row", "dE/seq", "dE/col")
FINE_NORMS = NORMS[1:]
SMALL_CAP, FINE_FACTOR, FINE_CAP, FINE_FLOOR = lc.SMALL_CAP, pm.FINE_FACTOR, pm.FINE_CAP, pm.FINE_FLOOR
assert set(pm.FINE_NORMS) == set(FINE_NORMS) and (FINE_FLOOR, FINE_FACTOR, FINE_CAP, SMALL_CAP) == (3e-4, 4.0, 1e-3, 0.05)
assert (pm.TENSOR_REL, pm.TENSOR_ABS) == (3e-4, 1e-6)

# G: "dense" | "label"; log: POST_LOG?; table: "gene" | "r2" | "r5" | "r16" | "empty" | "one"
Spec = collections.namedtuple("Spec", "models q b L emis G log eps seed table")

GENE_Q = (71, 127, 253)
DEG_Q = (65, 96, 128, 129, 192, 193, 256)                    # one .. four waves, one lane in the last wave, a full one
DEG_KINDS = ("deg0", "deg1", "deg2")
LENGTHS = (1, 2, 3, 7, 8, 9, 15, 16, 17, 33, 300)            # around PGW_PF = 4, WQ_PF = 8, WQ_T = 16 rows per group
BATCHES = (1, 3, 65, 130)                                    # (two groups: 33 = the first drain before the walk ends)
BATCH_L = 24
MODES = (False, True)
EMPTY_CLASS = 2


def spec_id(s):
    return "%s-q%d-b%d-L%d-%s-%s-%s-%s%s" % ("+".join(s.models), s.q, s.b, s.L, s.emis, s.G, s.table,
                                             "log" if s.log else "prob", "" if s.eps == EPS else "-eps%g" % s.eps)


def table_of(spec):
    """-> (list of q class indices, number of classes C); one table per (kind, q), whatever the seed."""
    return _table(spec.table, spec.q)


@functools.lru_cache(maxsize=None)
def _table(kind, q):
    rng = np.random.default_rng([77, q, len(kind)])
    if kind == "gene":
        return tuple(dm.gene_classes(q)), 6
    if kind == "one":
        return (0,) * q, 1
    if kind == "empty":
        return tuple(dm.random_map(rng, q, 5, empty=(EMPTY_CLASS,))), 5
    C = {"r2": 2, "r5": 5, "r16": 16}[kind]
    return tuple(dm.random_map(rng, q, C)), C


def one_hot(table, C, dtype=np.float64):
    M = np.zeros((len(table), C), dtype)
    M[np.arange(len(table)), np.asarray(table)] = 1
    return M


def build(spec):
    return _build(spec._replace(eps=EPS, log=False))         # neither eps nor the mode enters the draw


@functools.lru_cache(maxsize=None)
def _build(spec):
    q, b, L = spec.q, spec.b, spec.L
    k = len(spec.models)
    table, C = table_of(spec)
    rng = np.random.default_rng([spec.seed, q, b, L])
    Ms = [wc.model(rng, name, q) for name in spec.models]
    A, pi = np.stack([np.array(m[0]) for m in Ms]), np.stack([np.array(m[1]) for m in Ms])
    E = lc.draw_E(rng, spec.models, b, L, q, spec.emis)
    if spec.G == "dense":
        G = rng.standard_normal((k, b, L, C)).astype(np.float32)
    elif spec.G == "label":                                  # a cross-entropy against class labels
        used = np.flatnonzero(np.bincount(np.asarray(table), minlength=C))
        lab = used[rng.integers(0, len(used), (k, b, L))]
        G = -(lab[..., None] == np.arange(C)).astype(np.float32)
    else:
        raise ValueError(spec.G)
    out = dict(A=A, pi=pi, E=E, G=G)
    for v in out.values():
        v.flags.writeable = False
    return out


def expand(Gc, table):
    """The state-level upstream gradient (.., q) of a class-level one (.., C): G[..., j] = Gc[..., class(j)]."""
    return np.ascontiguousarray(np.asarray(Gc)[..., np.asarray(table)])


def oracle(A, pi, E, Gc, table, C, log, dtype=torch.float64, eps=EPS):
    """One model: (dA, dpi, dE, P) as fp64 numpy arrays: the gradient of sum Gc P (log=False) or sum Gc log P taken where
    Gc != 0 (log=True), by autograd in `dtype`; P (b,L,C) the class posteriors.  An empty class passes nothing."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)                                 # small matmuls: threads only cost
    try:
        A, pi, E = (torch.as_tensor(np.array(x), dtype=dtype).requires_grad_(True) for x in (A, pi, E))
        M = torch.as_tensor(one_hot(table, C), dtype=dtype)
        G = torch.as_tensor(np.array(Gc), dtype=dtype) * (M.sum(0) > 0)
        gam, _ = torch64.posterior(A, pi, E, eps)
        P = gam @ M
        on = G != 0
        out = torch.where(on, torch.log(torch.where(on, P, torch.ones_like(P))), torch.zeros_like(P)) if log else P
        (out * G).sum().backward()

        def grad(t):                                         # a length-1 sequence never touches A
            return np.asarray((torch.zeros_like(t) if t.grad is None else t.grad).numpy(), np.float64)
        return grad(A), grad(pi), grad(E), np.asarray(P.detach().numpy(), np.float64)
    finally:
        torch.set_num_threads(n)


def on_support(grads, A):
    return pc.on_support(grads, A)


def fine_norms(spec):
    """The relative norms a case is held to: none for the single class (this module's docstring)."""
    return () if spec.table == "one" else FINE_NORMS


@functools.lru_cache(maxsize=None)
def reference(spec):
    """-> list over the models of dict(want=(dA on the support, dpi, dE) fp64, P (b,L,C) fp64, e32, limit, small),
    read-only; None for a refused model."""
    c = build(spec)
    table, C = table_of(spec)
    out = []
    for m, name in enumerate(spec.models):
        if name == REFUSED:
            out.append(None)
            continue
        A, pi, E, G = c["A"][m], c["pi"][m], c["E"][m], c["G"][m]
        full = oracle(A, pi, E, G, table, C, spec.log, eps=spec.eps)
        want, P = on_support(full[:3], A), full[3]
        for x in want + (P,):
            x.flags.writeable = False
        twin = oracle(A, pi, E, G, table, C, spec.log, torch.float32, eps=spec.eps)
        e32, small = pm.errors(on_support(twin[:3], A), want, A)
        out.append(dict(want=want, P=P, e32=e32, small=small,
                        limit={n: max(FINE_FLOOR, FINE_FACTOR * e32[n]) for n in fine_norms(spec)}))
    return out


def check(got, ref_m, A):
    """(dA, dpi, dE) of one model -> ({norm: error}, {norm: limit}, off_support): how many entries of dA with A == 0
    are not exactly 0.0."""
    e, _ = pm.errors(tuple(np.asarray(x, np.float64) for x in got), ref_m["want"], A)
    off = int(np.count_nonzero(np.asarray(got[0])[np.asarray(A) == 0]))
    return e, pm.limits(ref_m), off


def engages(spec):
    return pc.engages(spec)                                  # (the models, emissions, eps and L decide)


def violations(spec):
    """The conditions of this module's docstring that `spec` misses, from the references alone ([] = none)."""
    c, bad = build(spec), []
    table, C = table_of(spec)
    used = np.bincount(np.asarray(table), minlength=C) > 0
    for m, ref in enumerate(reference(spec)):
        if ref is None:
            continue
        if not all(np.isfinite(x).all() for x in ref["want"]) or not all(np.isfinite(v) for v in ref["e32"].values()):
            bad.append((m, "not finite"))
        for n in fine_norms(spec):
            if not ref["small"][n] <= SMALL_CAP:
                bad.append((m, n, "small", ref["small"][n]))
            if not FINE_FACTOR * ref["e32"][n] <= FINE_CAP:
                bad.append((m, n, "e32", ref["e32"][n]))
        if spec.table == "one" and not ref["e32"]["tensor"] <= pm.TENSOR_REL:
            bad.append((m, "tensor", "e32", ref["e32"]["tensor"]))
        if spec.log:
            on = (c["G"][m] != 0) & used
            if on.any() and not ref["P"][on].min() >= MIN_P:
                bad.append((m, "min P", float(ref["P"][on].min())))
        _, count = pm.forward_backward64(c["A"][m], c["pi"][m], c["E"][m], eps=spec.eps)
        for clamp in engages(spec)[m]:
            if not count[clamp] >= 1:
                bad.append((m, clamp, "not engaged"))
    return bad


# ---- the cases ----------------------------------------------------------------------------------------------------
# Cases whose default seed does not meet the conditions of violations(), with the first seed of seed + 10, + 20, ...
# that does.  The 18-copy gene model: 4 e32 of dA/row = 2.4e-3 (rare, label, prob mode) and 5.1e-3 (dead, dense, log mode)
# at seed 1, and 1.3e-3 / 1.5e-3 at seeds 1 / 11 (holes, dense, prob mode; all under the suite's MKL_CBWR and
# ATEN_CPU_CAPABILITY settings, tests/conftest.py — the twin's rounding follows them).  The nine-copy batches in log mode with dense Gc: the smallest fp64 P_c among b L C = 9 360 / 18 720 entries
# was 8.2e-7 / 5.8e-7 at seed 4 (and 9.5e-7 at seed 14 for b = 130).
SEEDS = {"gene-q253-b3-L120-holes-dense-gene-prob": 21, "gene-q253-b3-L41-rare-label-gene-prob": 11, "gene-q253-b3-L41-dead-dense-gene-log": 11,
         "gene+deg2-q127-b65-L24-holes-dense-gene-log": 14, "gene-q127-b130-L24-holes-dense-gene-log": 24}


def seeded(specs):
    return [s._replace(seed=SEEDS.get(spec_id(s), s.seed)) for s in specs]


def both(models, q, b, L, emis, G, seed, table, eps=EPS):
    return [Spec(models, q, b, L, emis, G, log, eps, seed, table) for log in MODES]


def gene_sweep():
    out = []
    for q in GENE_Q:
        out += both(("gene",), q, 3, 120, "holes", "dense", 1, "gene")
        out += both(("gene",), q, 3, 41, "rare", "label", 1, "gene")
        out += both(("gene",), q, 3, 41, "dead", "dense", 1, "gene")
    return seeded(out)


def state_sweep():
    out = []
    for n, q in enumerate(DEG_Q):
        for i, kind in enumerate(DEG_KINDS):
            table = ("r16", "r2", "r5")[n % 3]               # 16 classes at 65, 129 and 256 states, with labels: a dense Gc
            G = "label" if table == "r16" else ("label", "dense")[(n + i) % 2]   # weighs log P of classes below MIN_P
            out += both((kind,), q, 3, 17, ("holes", "rare", "mid")[(n + i) % 3], G, 1, table)
    return seeded(out)


def length_sweep():
    return seeded([s for q, models, table in ((71, ("gene", "deg1"), "gene"), (193, ("deg2", "deg0"), "r16"))
                   for L in LENGTHS for s in both(models, q, 3, L, "holes", "dense", 2, table)])


def batch_sweep():
    return seeded([s for b in BATCHES
                   for s in both(("gene", "deg2") if b < 130 else ("gene",), 127, b, BATCH_L, "holes", "dense", 4, "gene")])


def eps_cases():
    """eps = 1e-6 with emissions between 1e-16 and 1e-6: the clamp is the caller's eps, not the default."""
    return seeded(both(("gene", "deg1"), 71, 4, 12, "mid", "dense", 7, "gene", eps=1e-6)
                  + both(("deg1",), 253, 4, 12, "mid", "label", 7, "r5", eps=1e-6)
                  + both(("gene",), 71, 3, 9, "dead", "dense", 7, "gene", eps=1e-6))


def table_cases():
    """An empty class (dense Gc: the engine is handed gradients for it and must pass nothing) and a single class."""
    return seeded(both(("gene", "deg1"), 71, 3, 17, "holes", "dense", 8, "empty")
                  + both(("deg2",), 129, 3, 17, "rare", "label", 8, "empty")
                  + both(("deg0",), 192, 3, 17, "holes", "label", 8, "one"))


def refused_cases():
    """A refused model next to a served one in one call, both modes."""
    return seeded(both((REFUSED, "deg1"), 96, 3, 17, "holes", "dense", 6, "r5"))


def all_specs():
    return gene_sweep() + state_sweep() + length_sweep() + batch_sweep() + eps_cases() + table_cases()
