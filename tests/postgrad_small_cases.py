"""Inputs, norms and routing predictions of the oracle sweep of hmm_posterior_grad for 1..16 states: the whole-sequence
sweeps (csrc/hmm_postgrad.inc, k_pg_fb<16> / k_pg_adj<16>) and the per-chunk path that is the shipped default there
(csrc/hmm_postgrad_chunked.inc: k_pc_values, k_pc_src, k_pc_scan, k_pc_final, k_pc_fold / k_pc_fold_seq).

Test infrastructure; imports neither the engine nor a GPU.  The norms, the oracle and the model builders are those of
tests/postgrad_mid_cases.py (imported, not copied).  tests/test_postgrad_small_cpu.py proves from the fp64 oracle alone
that these inputs can carry the comparison and that the table covers the edges it is for;
tests/test_postgrad_small_gpu.py runs the kernels on them.

A case is a Spec: the mid sweep's fields and T, the chunk length forced through HMM_OPT_CHUNK (0 = the engine's own).
build(spec) -> dict(A (k,q,q), pi (k,q), E (k,b,L,q), G (k,b,L,q)) float32, read-only, deterministic.
reference(spec) -> per model the fp64 oracle, its fp32 twin's error e32 under the four norms and the limits
(tensor 3e-4 + 1e-6; dE/col, dE/seq, dA/row max(3e-4, 4 e32)); with q = 1, where the oracle's gradient is identically
zero, `absolute`: max(1e-6, 4 x the twin's largest absolute entry) per tensor.
routing(spec) -> per model what the device-side rules of hmm_postgrad_chunked.inc must decide for each sequence, from
the fp64 recursion alone:
  F64      eps * sum_t 1 / Sg_t, Sg_t = <alpha_hat_t, Rb_t> (the certificate, threshold EXACT_DELTA = 2e-6);
  exposed  log mode: (F64 * sum_{gamma >= 1e-8} |G| / gamma + sum_{gamma < 1e-8} |G|) / sum |G| (threshold 1e-4);
  verdict  "chunk"  both rules clear their thresholds by a factor 4 and the support of A (entries > eps) is primitive,
           "whole"  a rule is exceeded by a factor 4, or the support is not primitive,
           "open"   everything else: fp32 sums may fall on either side, never asserted.
"""
import collections
import functools
import os

import numpy as np
import torch

import postgrad_mid_cases as pm
from oracle import params

EPS, SMALL = pm.EPS, pm.SMALL
TENSOR_REL, TENSOR_ABS = pm.TENSOR_REL, pm.TENSOR_ABS
FINE_FLOOR, FINE_FACTOR, FINE_CAP, FINE_NORMS = pm.FINE_FLOOR, pm.FINE_FACTOR, pm.FINE_CAP, pm.FINE_NORMS
ABSENT_REL = 2e-2                 # dA of absent edges through the per-chunk path (include/hmm_engine.h; tests/postgrad_sweep.py)
Q1_ABS, Q1_OF_G = 1e-6, 1e-3      # q = 1: the floor of the absolute bound, and what it must stay below (of max |G|)

EXACT_DELTA, PG_TINY_GAMMA, PC_LOG_EXPOSED = 2e-6, 1e-8, 1e-4        # hmm_engine.hip, hmm_postgrad.inc, hmm_postgrad_chunked.inc
MARGIN = 4.0
# the forward clamp on a PRIMITIVE model: k_topo_check reads the support as A > eps, so fclamp's edge of 1e-20 leaves
# its state D without a predecessor and the whole model to the whole-sequence sweeps.  With 1.25 eps the edge is in the
# support (by a quarter of eps, far from fp32 rounding of the comparison) and the predicted mass alpha_hat[0] * 1.25 eps
# is clamped wherever alpha_hat[0] <= 0.8: at nearly every position.
FCLAMP2_EDGE = 1.25e-16
PC_WARMUP, PC_FOLD_WAVES_MAX_SEQS, PC_MAX_SEQS, PC_MIN_CHUNKS, MAX_T = 64, 256, 4096, 4, 512

# model: "dense" | "sparse" (rand_model, primitive: tiny pi entries, no dead state) | "dense-d" | "sparse-d" (with states
# nothing enters: not primitive) | "triu" (upper triangular: reducible) | "gene" (params.intended_A15) | "simple7"
# (params.edges_simple) | "shipped" (A15_as_shipped of the transitioner fixture: eight all-zero rows) | "fclamp" |
# "fclamp2" (the same with an edge of FCLAMP2_EDGE, above eps: primitive) | "bclamp"; a tuple = that many models in one call.
# emis: "plain" | "holes" | "rare" | "dead" | "clamp" | "stretch".  G: "dense" | "label".
Spec = collections.namedtuple("Spec", "models q b L emis G log seed T")


def spec_id(s):
    return "%s-q%d-b%d-L%d-%s-%s-%s%s" % ("+".join(s.models), s.q, s.b, s.L, s.emis, s.G, "log" if s.log else "prob",
                                           "-T%d" % s.T if s.T else "")


def rand_counts(q):
    """(dead, tiny_pi) of rand_model for q states: the mid sweep's (3, 2) from 12 states on, fewer below."""
    return min(3, q // 4), min(2, q // 3)


@functools.lru_cache(maxsize=None)
def fixed_model(name):
    if name == "gene":
        A = params.intended_A15().numpy().astype(np.float32)
    else:
        with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "transitioner.npz")) as z:
            A = z["A15_as_shipped"].astype(np.float32)
    pi = np.full(15, 1 / 15, dtype=np.float32)
    A.flags.writeable = pi.flags.writeable = False
    return A, pi


def simple7_model(rng):
    """Random weights on the 15 edges of the 7-state topology (Ir, I0-2, E0-2)."""
    A = np.zeros((7, 7))
    ed = params.edges_simple()
    A[ed[:, 0], ed[:, 1]] = rng.random(len(ed)) + 0.1
    A /= A.sum(-1, keepdims=True)
    pi = rng.random(7) + 0.1
    pi /= pi.sum()
    return A.astype(np.float32), pi.astype(np.float32)


def build_model(rng, name, q):
    dead, tiny = rand_counts(q)
    if name in ("gene", "shipped"):
        assert q == 15
        return fixed_model(name)
    if name == "simple7":
        assert q == 7
        return simple7_model(rng)
    if name == "fclamp":
        return pm.forward_clamp_model(rng, q)
    if name == "fclamp2":
        A, pi = pm.forward_clamp_model(rng, q)
        A[0, q - 1] = FCLAMP2_EDGE                           # (after the row was normalised: its sum moves by 1e-16)
        return A, pi
    if name == "bclamp":
        return pm.backward_clamp_model(rng, q)
    if name == "triu":
        A, pi = pm.rand_model(rng, q, tiny_pi=tiny)
        A = np.triu(A).astype(np.float64)
        return (A / A.sum(-1, keepdims=True)).astype(np.float32), pi
    kind, _, d = name.partition("-")
    assert kind in ("dense", "sparse") and d in ("", "d"), name
    return pm.rand_model(rng, q, sparse=kind == "sparse", dead=dead if d else 0, tiny_pi=tiny)


def free_states(q):
    """The states whose emissions "rare" and "dead" leave alone: Ir, I, E of the gene model; Ir, I of the 7-state one."""
    return {15: 7, 7: 4}[q]


STRETCH = (1, 100, 120, 9)        # sequence, first and last + 1 position, the only state that emits there


def build(spec):
    """Spec -> dict(A, pi, E, G) float32 (read-only), the same arrays for the same spec in every process."""
    return _build(spec)


@functools.lru_cache(maxsize=None)
def _build(spec):
    k, q, b, L = len(spec.models), spec.q, spec.b, spec.L
    rng = np.random.default_rng([spec.seed, q, b, L, int(spec.log), spec.T])
    Ms = [build_model(rng, name, q) for name in spec.models]
    A, pi = np.stack([m[0] for m in Ms]), np.stack([m[1] for m in Ms])
    E = (rng.random((k, b, L, q)) * 0.9 + 0.05).astype(np.float32)
    if spec.emis == "plain":
        pass
    elif spec.emis == "holes":
        E[..., ::5, q // 3] = 0.0                            # emissions below eps: no gradient there
    elif spec.emis == "rare":
        rare = rng.random(E.shape) < 0.2
        rare[..., :free_states(q)] = False
        E[rare] = 1e-10                                      # far above eps: nothing is clamped
    elif spec.emis == "dead":                                # the emitter's magnitude, zeros in the constrained states
        E = E / np.float32(4096)
        dead = rng.random(E.shape) < 0.3
        dead[..., :free_states(q)] = False
        E[dead] = 0.0
    elif spec.emis == "clamp":
        for m, name in enumerate(spec.models):
            if name in ("fclamp", "fclamp2"):
                E[m, ..., q - 1] = 1.0
            elif name == "bclamp":
                E[m, ..., q - 1] = 0.0
    elif spec.emis == "stretch":                             # tests/test_postgrad_chunked_gpu.py::test_routing_per_model_and_per_sequence
        s, t0, t1, j = STRETCH
        E[0, s, t0:t1] = 0.0
        E[0, s, t0:t1, j] = 0.5
    else:
        raise ValueError(spec.emis)
    if spec.G == "dense":
        G = rng.standard_normal(E.shape).astype(np.float32)
    else:                                                    # a cross-entropy against the most probable state (fp64 gamma)
        G = np.empty_like(E)
        for m in range(k):
            gam = pm.forward_backward64(A[m], pi[m], E[m])[0]
            G[m] = -(gam == gam.max(-1, keepdims=True)).astype(np.float32)
    out = dict(A=A, pi=pi, E=E, G=G)
    for v in out.values():
        v.flags.writeable = False
    return out


@functools.lru_cache(maxsize=None)
def reference(spec):
    """-> list over the models of dict(want=(dA, dpi, dE) fp64, e32, limit, small as in the mid sweep, absolute=None or
    the q = 1 bound per tensor); computed once, read-only."""
    c = build(spec)
    out = []
    for m in range(len(spec.models)):
        want = pm.oracle(c["A"][m], c["pi"][m], c["E"][m], c["G"][m], spec.log)
        twin = pm.oracle(c["A"][m], c["pi"][m], c["E"][m], c["G"][m], spec.log, torch.float32)
        for x in want:
            x.flags.writeable = False
        e32, small = errors(twin, want, c["A"][m], False, floor_columns(spec.models[m], c["A"][m]))
        del e32["dA/absent"]
        e32_all_columns = pm.errors(twin, want, c["A"][m])[0]["dE/col"]
        limit = {n: max(FINE_FLOOR, FINE_FACTOR * e32[n]) for n in FINE_NORMS}
        absolute = [max(Q1_ABS, FINE_FACTOR * float(np.abs(x).max())) for x in twin] if spec.q == 1 else None
        # fp32 autograd through the recursion is not finite (the log-mode stretch): no limit can be derived from it, the
        # case keeps the tensor norm, whose limit is fixed
        norms = FINE_NORMS if all(np.isfinite(x).all() for x in twin) else ()
        out.append(dict(want=want, e32=e32, limit=limit, small=small, absolute=absolute, norms=norms,
                        e32_all_columns=e32_all_columns))
    return out


def limits(ref_m):
    return dict(ref_m["limit"], tensor=TENSOR_REL)


def floor_columns(name, A):
    """The state columns of dE that dE/col leaves to the tensor norm: for the as-shipped matrix the six states nothing
    enters.  They also have all-zero rows, so they sit on the eps floor at every position in both recursions, their
    columns are 1e-16 of the tensor and fp32 autograd itself is off by 1e8 relative there, whatever the seed: no
    per-column limit can be derived for them.  The other nine columns keep the norm."""
    if name != "shipped":
        return np.zeros(np.asarray(A).shape[-1], bool)
    return ~(np.asarray(A) > 0).any(0)


def errors(got, want, A, per_chunk, skip_cols=None):
    """pm.errors (dE/col over the columns not in skip_cols), and "dA/absent": the worst error of an absent edge's entry over the largest entry of the oracle's
    dA.  Whole-sequence runs hold those entries to the tensor norm; per-chunk runs (per_chunk=True) to ABSENT_REL, and
    their tensor norm of dA covers the present edges."""
    absent = np.asarray(A) <= 0
    dA, wA = np.asarray(got[0], np.float64), want[0]
    top = float(np.abs(wA).max())
    worst = float(np.abs(dA - wA)[absent].max()) / top if absent.any() and top > 0 else 0.0
    if per_chunk:
        got = (np.where(absent, wA, dA),) + tuple(got[1:])
    e, small = pm.errors(got, want, A)
    if skip_cols is not None and skip_cols.any():
        dE = np.array(got[2], np.float64)
        dE[..., skip_cols] = want[2][..., skip_cols]
        e2, small2 = pm.errors((got[0], got[1], dE), want, A)
        e["dE/col"], small["dE/col"] = e2["dE/col"], small2["dE/col"]
    e["dA/absent"] = worst
    return e, small


# ---- what the engine will do with a case --------------------------------------------------------------------------
def chunk_len(spec):
    """The chunk length of hmm_posterior_grad's per-chunk plan (pc_chunk_len over choose_T) for the case."""
    if spec.T:
        return spec.T
    NB, L = len(spec.models) * spec.b, spec.L
    lmax = (L + 15) // 16 * 16
    tb = 16
    while tb ** 3 * 4 < 9 * L and tb < MAX_T:
        tb += 16
    t = min(max((max(NB * L // 32768, tb) + 15) // 16 * 16, 16), MAX_T, lmax)
    ts = 16
    while ts * ts * 3 < 2 * L and ts < MAX_T:
        ts += 16
    return max(t, min(ts, lmax))


def chunks(spec):
    T = chunk_len(spec)
    return (spec.L + T - 1) // T


def last_chunk(spec):
    return spec.L - (chunks(spec) - 1) * chunk_len(spec)


def warmup_chunks(spec):
    T = chunk_len(spec)
    return (PC_WARMUP + T - 1) // T


def shipped_per_chunk(spec):
    """pc_wanted under HMM_OPT_PGCHUNK = 1 (q = 1: the engine returns exact zeros and runs no sweep at all)."""
    return spec.q > 1 and chunks(spec) >= PC_MIN_CHUNKS and len(spec.models) * spec.b <= PC_MAX_SEQS


def primitive(A, eps=EPS):
    """k_topo_check: the support of A (entries > eps) has a positive power (B^256 covers q <= 16)."""
    B = np.asarray(A) > eps
    for _ in range(8):
        B = (B.astype(np.int64) @ B.astype(np.int64)) > 0
    return bool(B.all())


@functools.lru_cache(maxsize=None)
def routing(spec):
    c = build(spec)
    out = []
    for m in range(len(spec.models)):
        gam, count, ah, Rb = pm.forward_backward64(c["A"][m], c["pi"][m], c["E"][m], parts=True)
        F = EPS * (1.0 / (ah * Rb).sum(-1)).sum(-1)                                  # (b,)
        ratio = F / EXACT_DELTA
        exposed = None
        if spec.log:
            w = np.abs(c["G"][m].astype(np.float64))
            tiny = gam < PG_TINY_GAMMA
            gp = np.where(tiny, 0.0, w / np.where(tiny, 1.0, gam)).sum((1, 2))
            exposed = (F * gp + np.where(tiny, w, 0.0).sum((1, 2))) / np.maximum(w.sum((1, 2)), 1e-300)
            ratio = np.maximum(ratio, exposed / PC_LOG_EXPOSED)
        prim = primitive(c["A"][m])
        verdict = ["whole" if (not prim or r >= MARGIN) else "chunk" if r <= 1 / MARGIN else "open" for r in ratio]
        out.append(dict(F=F, exposed=exposed, primitive=prim, verdict=verdict, count=count))
    return out


def serial_bounds(spec):
    """(fewest, most) sequences the whole-sequence sweeps serve under the shipped routing."""
    n = len(spec.models) * spec.b
    if not shipped_per_chunk(spec):
        return n, n
    v = [x for r in routing(spec) for x in r["verdict"]]
    return v.count("whole"), n - v.count("chunk")


def unclamped(spec):
    """No mixture clamp is active in the fp64 recursion: the cases HMM_OPT_PGCHUNK = 2 (no certificate) may serve."""
    return all(r["count"]["forward"] == 0 and r["count"]["backward"] == 0 for r in routing(spec))


def forced_per_chunk(spec):
    """The cases tests/test_postgrad_small_gpu.py also runs under HMM_OPT_PGCHUNK = 2: at least two chunks, primitive
    models and no mixture clamp in the fp64 recursion."""
    return spec.q > 1 and chunks(spec) >= 2 and unclamped(spec) and all(r["primitive"] for r in routing(spec))


# ---- the cases ----------------------------------------------------------------------------------------------------
MODES = (False, True)                                        # log?
SWEEP_B, SWEEP_L = 3, 203                                    # 25 prefetch blocks of MQ_PF = 8 positions, plus 3
LENGTHS = (1, 2, 3, 7, 8, 9, 15, 16, 17)
LENGTH_MODELS = {5: ("dense", "sparse"), 15: ("gene", "dense"), 16: ("dense", "sparse")}
GEOMETRY_MODELS = (("gene", 15), ("dense", 7), ("dense", 16))
GEOMETRY = ((16, (17, 33, 48, 49, 64, 65, 66, 79, 80, 129, 1041)), (48, (193,)), (64, (257,)), (80, (321,)))
BATCHES = (1, 64, 65, 130)

# Cases whose default seed does not meet the conditions of tests/test_postgrad_small_cpu.py, with the first seed of
# seed + 10, + 20, ... that does (the reason is next to each group).
SEEDS = {
    # a pi entry of 1e-20 on a state nothing enters: on the eps floor at every position, its dE column and dA row are
    # 1e-16 of their tensors and fp32 autograd is off by 1e4..1e8 relative there (as in the mid sweep)
    "dense-d-q7-b3-L203-holes-dense-prob": 11, "sparse-d-q8-b3-L203-holes-dense-prob": 11,
    "dense-d-q9-b3-L203-holes-dense-prob": 21, "dense-d-q11-b3-L203-holes-dense-prob": 11,
    "dense-d-q13-b3-L203-holes-dense-prob": 21, "sparse-d-q14-b3-L203-holes-dense-prob": 11,
    "dense-d-q15-b3-L203-holes-dense-prob": 21, "sparse-d-q16-b3-L203-holes-dense-prob": 11,
    # one sequence of the as-shipped model at 2e-5 of the tensor, and a dA row likewise: e32 3.6e-3 under both
    "gene+shipped-q15-b3-L203-plain-dense-prob-T16": 37,
    # a column of the as-shipped model that something enters at 1e-4 of the tensor: e32 of dE/col 8.7e-4
    "gene+shipped-q15-b3-L203-plain-label-log-T16": 27,
}


def grad_kind(log):
    """The upstream gradient of the cases that must be served per chunk.  In log mode a dense random gradient puts
    weight on the states whose posterior is below 1e-8 (every state with a pi entry of 1e-20 at t = 0, the gene model's
    improbable states anywhere), which the exposed-weight rule hands to the whole-sequence sweeps: there the gradient
    is the cross-entropy's, on the most probable state."""
    return "label" if log else "dense"


def seeded(specs):
    return [s._replace(seed=SEEDS.get(spec_id(s), s.seed)) for s in specs]


def state_sweep():
    out = []
    for log in MODES:
        for q in range(1, 17):                               # a primitive model for every q, dense and sparse alternating
            kind = "sparse" if q % 2 else "dense"
            out.append(Spec((kind,), q, SWEEP_B, SWEEP_L, "holes", "dense", log, 1, 0))
            if rand_counts(q)[0]:                            # ... and the other kind with states nothing enters
                other = "dense-d" if q % 2 else "sparse-d"
                out.append(Spec((other,), q, SWEEP_B, SWEEP_L, "holes", "dense", log, 1, 0))
        for name, q in (("gene", 15), ("simple7", 7)):
            out.append(Spec((name,), q, SWEEP_B, SWEEP_L, "holes", "dense", log, 1, 0))
            out.append(Spec((name,), q, SWEEP_B, SWEEP_L, "rare", "label", log, 1, 0))
            out.append(Spec((name,), q, SWEEP_B, SWEEP_L, "dead", "label", log, 1, 0))
    return seeded(out)


def length_sweep():
    return seeded([Spec(LENGTH_MODELS[q], q, 2, L, "holes", "dense", log, 2, 0) for log in MODES for q in (5, 15, 16)
                   for L in LENGTHS])


def geometry_sweep():
    return seeded([Spec((name,), q, 2, L, "plain", grad_kind(log), log, 5, T) for log in MODES for name, q in GEOMETRY_MODELS
                   for T, Ls in GEOMETRY for L in Ls])


def clamp_cases():
    out = [Spec((kind,), q, 3, 130, "clamp", "dense", log, 3, 16) for log in MODES for q in (6, 16)
           for kind in ("fclamp", "fclamp2", "bclamp")]
    out += [Spec(("gene",), 15, 3, SWEEP_L, "stretch", grad_kind(log), log, 3, 16) for log in MODES]
    return seeded(out)


def warmup_cases():
    """T = 64: the warm-up of k_pc_values is ONE chunk, so a warm-up that starts a chunk late is none at all.  The clamp
    constructions (the clamped state sits at every chunk boundary) and the gene model with rare emissions."""
    out = [Spec((kind,), q, 3, 257, "clamp", grad_kind(log), log, 8, 64) for log in MODES for q in (6, 16)
           for kind in ("fclamp2", "bclamp")]
    out += [Spec(("gene",), 15, 3, 257, emis, "label", log, 8, 64) for log in MODES for emis in ("rare", "dead")]
    return seeded(out)


def batch_sweep():
    """Whole-sequence: b on both sides of the 64-lane strides of k_pg_grad_sum / k_pg_sum_rows."""
    return seeded([Spec(("dense", "sparse"), 7, b, 24, "holes", "dense", log, 4, 0) for log in MODES for b in BATCHES])


def fold_cases():
    """Per chunk, C = 4: k b on both sides of PC_FOLD_WAVES_MAX_SEQS (k_pc_fold | k_pc_fold_seq), a reducible second
    model routed per model beside a per-chunk one, and both sides of the 4096-sequence cap of pc_wanted."""
    out = []
    for log in MODES:
        out.append(Spec(("dense", "sparse"), 5, 128, 64, "plain", grad_kind(log), log, 6, 16))
        out.append(Spec(("dense",), 5, 257, 64, "plain", grad_kind(log), log, 6, 16))
        out.append(Spec(("dense", "triu"), 5, 129, 64, "plain", grad_kind(log), log, 6, 16))
        out.append(Spec(("dense",), 3, 4096, 64, "plain", grad_kind(log), log, 6, 16))
        out.append(Spec(("dense",), 3, 4097, 64, "plain", grad_kind(log), log, 6, 16))
    return seeded(out)


def two_model_cases():
    """39 chains per model: a wave's four rows straddle the per-chunk model and the one redone whole."""
    return seeded([Spec(("gene", "shipped"), 15, SWEEP_B, SWEEP_L, "plain", grad_kind(log), log, 7, 16) for log in MODES])


def all_specs():
    return (state_sweep() + length_sweep() + geometry_sweep() + clamp_cases() + batch_sweep() + fold_cases()
            + two_model_cases() + warmup_cases())


def engages(spec):
    """The clamps a case must engage in the fp64 recursion (per model: set of forward / backward / pi / E)."""
    out = []
    for name in spec.models:
        s = set()
        if spec.emis in ("holes", "dead", "stretch"):
            s.add("E")
        if name.split("-")[0] in ("dense", "sparse", "triu") and rand_counts(spec.q)[1]:
            s.add("pi")
        if name.endswith("-d") and spec.L >= 100:            # dead states keep half their mass per step
            s.add("forward")
        if name in ("fclamp", "fclamp2"):
            s.add("forward")
        if name == "bclamp":
            s |= {"backward", "E"}
        if name == "shipped":
            s |= {"forward", "backward"}
        out.append(s)
    return out
