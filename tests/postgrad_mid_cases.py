"""Inputs and norms of the oracle sweep of hmm_posterior_grad for 17..64 states (the whole-sequence sweeps of
csrc/hmm_postgrad.inc: k_pg_fb<QB>, k_pg_adj<QB>, k_pg_merge, k_pg_grad_sum, k_pg_sum_rows with QB = 32, 48, 64).

Test infrastructure; imports neither the engine nor a GPU.  tests/test_postgrad_mid_cpu.py proves from the fp64 oracle
alone that these inputs can carry the comparison (finite gradients, clamps engaged, fp32 rounding far below the limit);
tests/test_postgrad_mid_gpu.py runs the kernels on them.

A case is a Spec; build(spec) -> dict(A (k,q,q), pi (k,q), E (k,b,L,q), G (k,b,L,q)) float32, deterministic.
reference(spec) -> per model the fp64 oracle (oracle/torch64.py) and its fp32 twin (the same recursion and autograd
with float32 tensors on the CPU), both cached for the process and read-only.

Four norms.  A gradient is held to the oracle under
  tensor    max|err| <= 3e-4 max|want| + 1e-6 for each of dA, dpi, dE (the project's norm, fixed);
  dE/col    max over (b, t) of |err| in state column j / max|want| in column j, worst j;
  dE/seq    the same per sequence;
  dA/row    row i over its present edges (A > 0) / max|want| over those edges, worst i (absent edges of a row are held
            to the tensor norm: the reference never reads them, tests/test_grad_gpu.py).
A column, sequence or row whose reference scale is below SMALL = 1e-30 of the tensor's maximum is held to the tensor
norm only; at most 5 % of a case's columns / rows may be (asserted by the CPU test).  The limit of the three finer norms
is max(3e-4, 4 e32) per case, model and norm, e32 being the fp32 twin's error under that norm: the factor 4 pays for the
kernel's approximate reciprocals (v_rcp_f32, 1 ulp) and its different summation order.
"""
import collections
import functools
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch

from oracle import torch64

EPS = 1e-16
SMALL = 1e-30
TENSOR_REL, TENSOR_ABS = 3e-4, 1e-6
FINE_FLOOR, FINE_FACTOR, FINE_CAP = 3e-4, 4.0, 1e-3
FINE_NORMS = ("dE/col", "dE/seq", "dA/row")

# model: "dense" | "sparse" (rand_model with dead=3, tiny_pi=2) | "gene" (1 + 14 c states) | "fclamp" | "bclamp";
# a tuple of names = that many models in one call.  emis: "holes" | "rare" | "dead" | "clamp".  G: "dense" | "label".
Spec = collections.namedtuple("Spec", "models q b L emis G log seed")


def spec_id(s):
    return "%s-q%d-b%d-L%d-%s-%s-%s" % ("+".join(s.models), s.q, s.b, s.L, s.emis, s.G, "log" if s.log else "prob")


def rand_model(rng, q, sparse=False, dead=0, tiny_pi=0):
    """Row-stochastic A; `dead` states nothing enters; `tiny_pi` entries of pi below eps."""
    A = rng.random((q, q)) ** 2 + 1e-2
    if sparse:
        A *= rng.random((q, q)) < 0.1
        A += np.eye(q) * 0.3
        A[np.arange(q), (np.arange(q) + 1) % q] += 0.2
    if dead:
        A[:, q - dead:] = 0.0
        A[q - dead:, q - dead:] = np.eye(dead) * 0.5
        A[q - dead:, 0] += 0.5
    A /= A.sum(-1, keepdims=True)
    pi = rng.random(q) + 0.1
    if tiny_pi:
        pi[rng.choice(q, tiny_pi, replace=False)] = 1e-20
    pi /= pi.sum()
    return A.astype(np.float32), pi.astype(np.float32)


@functools.lru_cache(maxsize=None)
def gene_model(copies):
    """(A, pi) of the `copies`-copy gene model (1 + 14 copies states) with its own initial distribution."""
    from hmm_layer_amd.gene_pred_hmm_transitioner import GenePredMultiHMMTransitioner
    tr = GenePredMultiHMMTransitioner(k=copies, initial_exon_len=200, initial_intron_len=4500, initial_ir_len=10000)
    with torch.no_grad():
        A = tr.make_A()[0].numpy().astype(np.float32)
        pi = tr.make_initial_distribution().reshape(-1).numpy().astype(np.float32)
    A.flags.writeable = pi.flags.writeable = False
    return A, pi


def forward_clamp_model(rng, q, edge=1e-20):
    """tests/test_posterior_grad_large_gpu.py::test_clamped_predicted_state: state D = q - 1 is entered by a PRESENT
    edge 0 -> D of weight 1e-20 alone and emits with probability 1 (build()), so the forward cell clamps its predicted
    mass at every position t >= 1.  One departure from that test: pi[D] is not 0.  With pi[D] = 0 the state sits on the
    floor at t = 0 as well, its dE column and its dA row are 1e-16 of their tensors in POST_PROB, and fp32 autograd
    itself is off by a factor 1e7 there (e32 of dE/col and dA/row): the finer norms would say nothing.  With mass at
    t = 0 that column and row have a scale, and the clamp is as active as before."""
    D = q - 1
    A = rng.random((q, q)) ** 2 + 1e-2
    A[:, D] = 0.0
    A[0, D] = edge
    A[D, :] = 0.0
    A[D, 0] = 1.0
    A /= A.sum(-1, keepdims=True)
    pi = rng.random(q) + 0.1
    pi /= pi.sum()
    return A.astype(np.float32), pi.astype(np.float32)


def backward_clamp_model(rng, q):
    """State X = q - 2 has the single successor Z = q - 1, which never emits (build() zeroes E[..., Z]): bh_{t+1}[Z] is
    eps * Rb[Z] / Sb, far below eps, so (A bh)[X] is clamped at every position but the last."""
    X, Z = q - 2, q - 1
    A = rng.random((q, q)) ** 2 + 1e-2
    A[X, :] = 0.0
    A[X, Z] = 1.0
    A /= A.sum(-1, keepdims=True)
    pi = rng.random(q) + 0.1
    pi /= pi.sum()
    return A.astype(np.float32), pi.astype(np.float32)


def copies_of(q):
    assert (q - 1) % 14 == 0, q
    return (q - 1) // 14


def build_model(rng, name, q):
    if name == "gene":
        return gene_model(copies_of(q))
    if name == "fclamp":
        return forward_clamp_model(rng, q)
    if name == "bclamp":
        return backward_clamp_model(rng, q)
    return rand_model(rng, q, sparse=name == "sparse", dead=3, tiny_pi=2)


def forward_backward64(A, pi, E, eps=EPS, parts=False):
    """The recursion of oracle/torch64.posterior restated in numpy fp64 with its intermediates: gamma (b,L,q) and how
    often each clamp is active: forward predicted state <= eps (t >= 1), A bh <= eps, pi <= eps, E <= eps.
    parts=True: also alpha_hat and Rb (b,L,q), whose products are gamma before it is normalised."""
    A, pi, E = np.asarray(A, np.float64), np.asarray(pi, np.float64), np.asarray(E, np.float64)
    b, L, q = E.shape
    Ec = np.maximum(E, eps)
    ah, Rb = np.empty((b, L, q)), np.empty((b, L, q))
    n_fwd = n_bwd = 0
    state = np.broadcast_to(pi, (b, q))
    for t in range(L):
        R = state if t == 0 else state @ A
        if t:
            n_fwd += int((R <= eps).sum())
        sf = Ec[:, t] * np.maximum(R, eps)
        state = sf / sf.sum(-1, keepdims=True)
        ah[:, t] = state
    bh = None
    for t in range(L - 1, -1, -1):
        if t == L - 1:
            R = np.ones((b, q))
        else:
            raw = bh @ A.T
            n_bwd += int((raw <= eps).sum())
            R = np.maximum(raw, eps)
        Rb[:, t] = R
        sb = Ec[:, t] * R
        bh = sb / sb.sum(-1, keepdims=True)
    g = ah * Rb
    count = dict(forward=n_fwd, backward=n_bwd, pi=int((pi <= eps).sum()) * b, E=int((E <= eps).sum()))
    return (g / g.sum(-1, keepdims=True), count) + ((ah, Rb) if parts else ())


def build(spec):
    """Spec -> dict(A, pi, E, G) float32 (read-only), the same arrays for the same spec in every process."""
    return _build(spec)


@functools.lru_cache(maxsize=None)
def _build(spec):
    k, q, b, L = len(spec.models), spec.q, spec.b, spec.L
    rng = np.random.default_rng([spec.seed, q, b, L, int(spec.log)])
    Ms = [build_model(rng, name, q) for name in spec.models]
    A, pi = np.stack([m[0] for m in Ms]), np.stack([m[1] for m in Ms])
    E = (rng.random((k, b, L, q)) * 0.9 + 0.05).astype(np.float32)
    if spec.emis == "holes":
        E[..., ::5, q // 3] = 0.0                            # emissions below eps: no gradient there
    elif spec.emis == "rare":
        rare = rng.random(E.shape) < 0.2
        rare[..., :7] = False
        E[rare] = 1e-10                                      # far above eps: nothing is clamped
    elif spec.emis == "dead":                                # the emitter's magnitude, zeros in the constrained states
        E = E / np.float32(4096)
        dead = rng.random(E.shape) < 0.3
        dead[..., :1 + 6 * copies_of(q)] = False
        E[dead] = 0.0
    elif spec.emis == "clamp":
        for m, name in enumerate(spec.models):
            if name == "fclamp":
                E[m, ..., q - 1] = 1.0
            elif name == "bclamp":
                E[m, ..., q - 1] = 0.0
    else:
        raise ValueError(spec.emis)
    if spec.G == "dense":
        G = rng.standard_normal(E.shape).astype(np.float32)
    else:                                                    # a cross-entropy against the most probable state (fp64 gamma)
        G = np.empty_like(E)
        for m in range(k):
            gam = forward_backward64(A[m], pi[m], E[m])[0]
            G[m] = -(gam == gam.max(-1, keepdims=True)).astype(np.float32)
    out = dict(A=A, pi=pi, E=E, G=G)
    for v in out.values():
        v.flags.writeable = False
    return out


def oracle(A, pi, E, G, log, dtype=torch.float64, eps=EPS, add_loglik=False):
    """One model: (dA, dpi, dE) of <G, gamma | log gamma> as fp64 numpy arrays, by autograd in `dtype`."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)                                 # small matmuls: threads only cost
    try:
        A, pi, E, G = (np.array(x) for x in (A, pi, E, G))     # writable copies of the read-only inputs
        out = torch64.posterior_grad(A, pi, E, G, log=log, eps=eps, add_loglik=add_loglik, dtype=dtype)
        return tuple(np.asarray(x, np.float64) for x in out[:3])
    finally:
        torch.set_num_threads(n)


@functools.lru_cache(maxsize=None)
def reference(spec):
    """-> list over the models of dict(want=(dA, dpi, dE) fp64, e32={norm: fp32 twin's error}, limit={norm: limit},
    small={norm: fraction of columns / rows under the tensor norm only}); computed once, read-only."""
    c = build(spec)
    out = []
    for m in range(len(spec.models)):
        want = oracle(c["A"][m], c["pi"][m], c["E"][m], c["G"][m], spec.log)
        twin = oracle(c["A"][m], c["pi"][m], c["E"][m], c["G"][m], spec.log, torch.float32)
        for x in want:
            x.flags.writeable = False
        e32, small = errors(twin, want, c["A"][m])
        limit = {n: max(FINE_FLOOR, FINE_FACTOR * e32[n]) for n in FINE_NORMS}
        out.append(dict(want=want, e32=e32, limit=limit, small=small))
    return out


def _ratio(err, scale, top):
    """max of err / scale over the entries whose scale is at least SMALL * top; the fraction of entries below."""
    ok = scale >= SMALL * top
    if top == 0.0 or not ok.any():
        return 0.0, float(1.0 - ok.mean())
    return float((err[ok] / scale[ok]).max()), float(1.0 - ok.mean())


def errors(got, want, A):
    """(dA, dpi, dE) of one model against the oracle's -> ({norm: error}, {fine norm: fraction under the small-scale
    rule}).  "tensor" is the worst of (max|err| - 1e-6) / max|want| over the three tensors (<= 3e-4 passes)."""
    e, small = {}, {}
    e["tensor"] = max((np.abs(g - w).max() - TENSOR_ABS) / max(np.abs(w).max(), 1e-300) for g, w in zip(got, want))
    dE, wE = np.asarray(got[2], np.float64), want[2]
    err, ref = np.abs(dE - wE), np.abs(wE)
    top = float(ref.max())
    e["dE/col"], small["dE/col"] = _ratio(err.max((0, 1)), ref.max((0, 1)), top)
    e["dE/seq"], small["dE/seq"] = _ratio(err.max((1, 2)), ref.max((1, 2)), top)
    dA, wA = np.asarray(got[0], np.float64), want[0]
    present = np.asarray(A) > 0
    err, ref = np.where(present, np.abs(dA - wA), 0.0), np.where(present, np.abs(wA), 0.0)
    e["dA/row"], small["dA/row"] = _ratio(err.max(-1), ref.max(-1), float(np.abs(wA).max()))
    return e, small


def limits(ref_m):
    return dict(ref_m["limit"], tensor=TENSOR_REL)


# ---- the cases ----------------------------------------------------------------------------------------------------
STATE_Q = (17, 31, 32, 33, 47, 48, 49, 63, 64)               # both ends of QB = 32, 48, 64 and inactive lanes in each
GENE_Q = (29, 43, 57)
SWEEP_B, SWEEP_L = 3, 203                                    # 25 prefetch blocks of MQ_PF = 8 positions, plus 3
LENGTHS = (1, 2, 3, 7, 8, 9, 15, 16, 17)                     # around one and two prefetch blocks
LENGTH_MODELS = {33: ("dense", "sparse"), 43: ("gene", "dense"), 57: ("gene", "sparse")}
BATCHES = (1, 64, 65, 130)                                   # the 64-lane strides of k_pg_grad_sum / k_pg_sum_rows
MODES = (False, True)                                        # log?


# Cases whose default seed does not meet the conditions of tests/test_postgrad_mid_cpu.py, with the first seed of
# seed + 10, + 20, ... that does.  In the POST_PROB cases the draw put a pi entry of 1e-20 on one of the three states
# nothing enters: that state is on the eps floor at every position, its dE column and dA row are 1e-16 of their
# tensors, and fp32 autograd is off by 1e6..1e7 relative there (e32).  In the two POST_LOG cases a gene-model row of dA
# is 1e-7 of the tensor and 4 e32 of dA/row came to 3.5e-2 and 1.6e-3.
SEEDS = {
    "dense-q17-b3-L203-holes-dense-prob": 31, "sparse-q31-b3-L203-holes-dense-prob": 11,
    "dense-q64-b3-L203-holes-dense-prob": 11, "gene-q57-b3-L203-rare-label-log": 11,
    "dense+sparse-q33-b2-L3-holes-dense-prob": 22, "dense+sparse-q33-b2-L8-holes-dense-prob": 12,
    "dense+sparse-q33-b2-L15-holes-dense-prob": 12, "gene+dense-q43-b2-L2-holes-dense-prob": 12,
    "gene+dense-q43-b2-L9-holes-dense-prob": 12, "gene+dense-q43-b2-L16-holes-dense-prob": 12,
    "gene+dense-q43-b2-L3-holes-dense-log": 12,
}


def seeded(specs):
    return [s._replace(seed=SEEDS.get(spec_id(s), s.seed)) for s in specs]


def state_sweep():
    out = []
    for log in MODES:
        for n, q in enumerate(STATE_Q):
            out.append(Spec(("sparse" if n % 2 else "dense",), q, SWEEP_B, SWEEP_L, "holes", "dense", log, 1))
        for q in GENE_Q:
            out.append(Spec(("gene",), q, SWEEP_B, SWEEP_L, "holes", "dense", log, 1))
            out.append(Spec(("gene",), q, SWEEP_B, SWEEP_L, "rare", "label", log, 1))
            out.append(Spec(("gene",), q, SWEEP_B, SWEEP_L, "dead", "label", log, 1))
    return seeded(out)


def length_sweep():
    return seeded([Spec(LENGTH_MODELS[q], q, 2, L, "holes", "dense", log, 2) for log in MODES for q in (33, 43, 57)
                   for L in LENGTHS])


def clamp_cases():
    return [Spec((kind,), q, 3, 60, "clamp", "dense", log, 3) for log in MODES for q in (40, 60)
            for kind in ("fclamp", "bclamp")]


def batch_sweep():
    return [Spec(("gene", "sparse"), 43, b, 24, "holes", "dense", log, 4) for log in MODES for b in BATCHES]


def all_specs():
    return state_sweep() + length_sweep() + clamp_cases() + batch_sweep()


def engages(spec):
    """The clamps a case must engage in the fp64 recursion (per model: list of sets of forward / backward / pi / E)."""
    out = []
    for name in spec.models:
        s = set()
        if spec.emis in ("holes", "dead"):
            s.add("E")
        if name in ("dense", "sparse"):                      # tiny_pi=2; dead=3: they keep half their mass per step
            s.add("pi")
            if spec.L >= 100:
                s.add("forward")
        if name == "fclamp":
            s.add("forward")
        if name == "bclamp":
            s |= {"backward", "E"}
        out.append(s)
    return out
