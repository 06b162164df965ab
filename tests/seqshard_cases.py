"""Inputs, norms and drivers of the oracle sweep of the sequence-sharded posterior (hmm_seqshard_reduce /
hmm_seqshard_posterior, csrc/hmm_seqshard.inc, driven by hmm_layer_amd/seqshard.py).

Test infrastructure; imports neither the engine nor a GPU at module level (sharded() imports them when called).
tests/test_seqshard_sweep_cpu.py proves from the fp64 restatement (tests/seqshard_ref.py) and the oracle alone that
these inputs can carry the comparison; tests/test_seqshard_sweep_gpu.py runs the kernels on them.

Models (model(name) -> A (k,q,q), pi (k,q) float32, read-only):
  "d1" .. "d16"   dense random models (rand_model of tests/test_engine_gpu.py), one per state count
  "d15b"          a second dense 15-state model with its own matrix
  "g7"            the 7-state gene topology (compiled: TopoGene7), length-based transition probabilities
  "g15"           the 15-state gene model params.intended_A15() (compiled: TopoGene15)
  "a+b"           two models in one call
  "...@hot"       the same model with a one-hot start distribution (state 0)
  "shipped15", "eye12", "g7absent"   models whose support is not primitive (section C only)

"g7absent" is params.dense_A(edges_simple(), init_logits(...), 7, zero_logit_is_absent=True): with the zero logits
taken as absent edges every intron state and the intergenic state keep their self-loop alone, the chain is reducible,
and no compiled topology or scan serves it (phi = +inf).  The sweep's 7-state gene model therefore keeps those edges.

Section A: the slab operator alone.  a_cases() -> ASpec(model, Ls, seq_start, variant, chunk); a_build(spec) -> E
(k,3,Ls,q); a_reference(spec) -> RefBackend.reduce's operator, op32's, e32 and the limit max(4 e32, 1e-6).
Section B: benign inputs end to end.  b_cases(); b_build(spec) -> E (k,3,L,q).
Section C: hard inputs.  c_build(name) -> E (1,b,96,q) and one Hard record per sequence; ROBUST is the set of
(model, sequence) pairs whose reference verdict survives perturbation (certify()), stored as a literal and re-derived by
the CPU test.
"""
import collections
import functools
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch

from oracle import params

from seqshard_ref import RefBackend

EPS = 1e-16
PHI_LIMIT = 2e-6                                             # seqshard.PHI_LIMIT (asserted equal by the CPU test)
TOL_FLOOR, TOL_FACTOR, TOL_CAP = 1e-6, 4.0, 1e-4             # section A: limit = max(4 e32, 1e-6), and 4 e32 < 1e-4
GAMMA_TOL, UNSHARDED_TOL = 2e-5, 2e-6                        # tests/test_seqshard_gpu.py
LL_REL, LL_ABS = 1e-6, 2e-4
NO_LL_REL = 2.4e-7                                           # POST_LOG_NO_LL: fp32 log values of the log-likelihood's size
B = 3


def _frozen(*xs):
    for x in xs:
        x.flags.writeable = False
    return xs


def rand_model(rng, q):
    """tests/test_engine_gpu.py::rand_model (dense)."""
    A = rng.random((q, q)) ** 3 + 1e-3
    A /= A.sum(-1, keepdims=True)
    pi = rng.random(q) + 0.1
    pi /= pi.sum()
    return A.astype(np.float32), pi.astype(np.float32)


def primitive(A, eps=EPS):
    """Is the support of A (entries > eps) primitive: some power of it is positive (k_topo_check's question)."""
    S = np.asarray(A) > eps
    P = S.copy()
    for _ in range(8):                                       # S^256: Wielandt's bound for q <= 16 is (q-1)^2 + 1 = 226
        P = (P.astype(np.int64) @ P.astype(np.int64)) > 0
    return bool(P.all())


@functools.lru_cache(maxsize=None)
def _single(name):
    hot = name.endswith("@hot")
    base = name[:-4] if hot else name
    if base == "g15":
        A, pi = params.intended_A15().numpy().astype(np.float32), np.full(15, 1 / 15, dtype=np.float32)
    elif base in ("g7", "g7absent"):
        ed = params.edges_simple()
        A = params.dense_A(ed, params.init_logits(ed, 1, 200, 4500, 10000), 7,
                           zero_logit_is_absent=base == "g7absent").numpy().astype(np.float32)
        pi = np.full(7, 1 / 7, dtype=np.float32)
    elif base == "shipped15":
        with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "transitioner.npz")) as z:
            A = z["A15_as_shipped"].astype(np.float32)
        pi = np.full(15, 1 / 15, dtype=np.float32)
    elif base == "eye12":
        A, pi = np.eye(12, dtype=np.float32), np.full(12, 1 / 12, dtype=np.float32)
    elif base == "d15b":
        A, pi = rand_model(np.random.default_rng([11, 15, 2]), 15)
    else:
        assert base[0] == "d", name
        q = int(base[1:])
        A, pi = rand_model(np.random.default_rng([11, q]), q)
    if hot:
        pi = np.zeros_like(pi)
        pi[0] = 1.0
    return _frozen(A, pi)


@functools.lru_cache(maxsize=None)
def model(name):
    Ms = [_single(n) for n in name.split("+")]
    return _frozen(np.stack([m[0] for m in Ms]), np.stack([m[1] for m in Ms]))


def compiled(name):
    """Does a model of the call run on a compiled topology (sparse reduce) when OPT_FORCE_DENSE = 0?"""
    return any(n.split("@")[0] in ("g7", "g15") for n in name.split("+"))


DENSE = tuple("d%d" % q for q in range(1, 17))
GENE = ("g7", "g15")
TWO = ("g15+d15", "d15+d15b")                                # sparse waves straddling two models; two dense matrices
SWEEP_MODELS = DENSE + GENE + TWO
LONG_MODELS = ("d5", "d16", "g7", "g15")


# ---- the fp64 restatement over a list of cuts, and its fp32 twin of the reduce ------------------------------------
def ref_run(A, pi, E, cuts):
    """RefBackend over the slabs E[:, :, cuts[r]:cuts[r+1]]: reduce on every slab, stack, posterior on every slab.
    -> out (k,b,L,q) float32, [ll (k,b) per rank], [phi (k,b) per rank]."""
    be = RefBackend()
    R = len(cuts) - 1
    At, pit = torch.from_numpy(np.array(A)), torch.from_numpy(np.array(pi))
    slabs = [torch.from_numpy(np.array(E[:, :, cuts[r]:cuts[r + 1]])) for r in range(R)]
    red = [be.reduce(At, slabs[r], r == 0, R) for r in range(R)]
    ops = torch.stack([o for o, _ in red], dim=2).contiguous()
    exs = torch.stack([e for _, e in red], dim=2).contiguous()
    outs, lls, phis = [], [], []
    for r in range(R):
        o, ll, ph = be.posterior(At, pit, slabs[r], ops, exs, r, 0)
        outs.append(o.numpy())
        lls.append(ll.numpy())
        phis.append(ph.numpy())
    return np.concatenate(outs, axis=2), lls, phis


def op32(A, E_slab, seq_start):
    """The slab operator formed step by step in float32 numpy: RefBackend.reduce's recurrence and per-step
    power-of-two column rescale.  -> op (k,b,16,16) float32, ex (k,b,16) int32."""
    A, E = np.asarray(A, np.float32), np.asarray(E_slab, np.float32)
    k, b, L, q = E.shape
    At = np.ascontiguousarray(np.swapaxes(A, 1, 2))[:, None]                     # (k,1,q,q)
    X = np.broadcast_to(np.eye(q, dtype=np.float32), (k, b, q, q)).copy()
    e = np.zeros((k, b, q), np.int64)
    for t in range(L):
        em = np.maximum(E[:, :, t], np.float32(EPS))
        X = em[..., None] * (X if (t == 0 and seq_start) else np.matmul(At, X))
        assert X.dtype == np.float32
        s = X.sum(-2)
        xe = np.where(s > 0, np.frexp(np.where(s > 0, s, np.float32(1)))[1], 0)
        X = X * np.ldexp(np.float32(1), -xe)[..., None, :].astype(np.float32)
        e = e + xe
    op = np.zeros((k, b, 16, 16), np.float32)
    ex = np.zeros((k, b, 16), np.int32)
    op[..., :q, :q] = X
    ex[..., :q] = e
    return op, ex


def op_error(op, ex, op_ref, ex_ref, q):
    """max over sequences and columns n < q of |op[:, n] 2^(ex[n] - ex_ref[n]) - op_ref[:, n]| / max_i op_ref[i, n]:
    the leading q x q block and the first q exponents only."""
    a = np.asarray(op, np.float64)[..., :q, :q]
    r = np.asarray(op_ref, np.float64)[..., :q, :q]
    d = (np.asarray(ex, np.int64) - np.asarray(ex_ref, np.int64))[..., :q]
    with np.errstate(over="ignore", invalid="ignore"):
        err = np.abs(a * np.ldexp(1.0, np.clip(d, -2000, 2000))[..., None, :] - r).max(-2)
    top = r.max(-2)
    if not (np.isfinite(err).all() and (top > 0).all()):
        return float("inf")
    return float((err / top).max())


# ---- section A ------------------------------------------------------------------------------------------------------
ASpec = collections.namedtuple("ASpec", "model Ls seq_start variant chunk")
SHORT_LS = (1, 2, 15, 16, 17, 33, 100)                       # default chunk length (16 at these sizes): 1 .. 7 chunks
LONG_LS = (496, 511, 512, 513, 1000)                         # OPT_CHUNK = 16: 31, 32, 32, 33, 63 chunks
VARIANTS = ("plain", "dead", "tiny")


def a_id(s):
    return "%s-Ls%d-start%d-%s-chunk%d" % s


def a_cases(models=None):
    out = [ASpec(m, Ls, ss, v, 0) for m in SWEEP_MODELS for Ls in SHORT_LS for ss in (0, 1) for v in VARIANTS]
    out += [ASpec(m, Ls, ss, v, 16) for m in LONG_MODELS for Ls in LONG_LS for ss in (0, 1) for v in VARIANTS]
    return [s for s in out if models is None or s.model in models]


def tiny_states(q):
    return sorted({0, q // 2, q - 1})


def a_build(spec):
    return _a_build(spec)


@functools.lru_cache(maxsize=None)
def _a_build(spec):
    """E (k,3,Ls,q): uniform in [0.05, 0.95]; "dead": state q // 2 emits exact zeros throughout; "tiny": every
    emission is scaled by 1e-10 and three states emit 1e-10 flat, so that every step takes 2^-33 or more off every
    column (1000 positions: exponents beyond -33000) without any column leaving fp32's normal range between two sums."""
    A, _ = model(spec.model)
    k, q = A.shape[:2]
    rng = np.random.default_rng([21, SWEEP_MODELS.index(spec.model), spec.Ls, spec.seq_start,
                                 VARIANTS.index(spec.variant)])
    E = (rng.random((k, B, spec.Ls, q)) * 0.9 + 0.05).astype(np.float32)
    if spec.variant == "dead":
        E[..., q // 2] = 0.0
    elif spec.variant == "tiny":
        E *= np.float32(1e-10)
        E[..., tiny_states(q)] = 1e-10
    return _frozen(E)[0]


@functools.lru_cache(maxsize=None)
def a_reference(spec):
    """-> dict(op, ex: RefBackend.reduce; e32: op32's error against it; limit)."""
    A, _ = model(spec.model)
    E = a_build(spec)
    op, ex = RefBackend().reduce(torch.from_numpy(np.array(A)), torch.from_numpy(np.array(E)), spec.seq_start, 1)
    op, ex = op.numpy(), ex.numpy()
    o32, x32 = op32(A, E, spec.seq_start)
    e32 = op_error(o32, x32, op, ex, A.shape[-1])
    return dict(op=op, ex=ex, e32=e32, limit=max(TOL_FACTOR * e32, TOL_FLOOR))


# ---- section B ------------------------------------------------------------------------------------------------------
BSpec = collections.namedtuple("BSpec", "model L cuts")
B_L = 203
B_CUTS = ((0, B_L), (0, 1, B_L), (0, B_L - 1, B_L), (0, 101, B_L), (0, 100, 101, B_L), (0, 16, 33, 48, 117, B_L),
          (0, 1, 2, 3, 4, 5, 6, 7, B_L))
B_MODELS = SWEEP_MODELS + ("d5@hot", "g15@hot")
B_LONG = BSpec(None, 1513, (0, 513, 1513))                   # 33 and 63 chunks of 16: both slabs compose in two levels
B_LONG_MODELS = ("g7", "g15", "d16")


def b_id(s):
    return "%s-L%d-cuts%s" % (s.model, s.L, "_".join(str(c) for c in s.cuts[1:-1]) or "none")


def b_cases(models=None):
    out = [BSpec(m, B_L, c) for m in B_MODELS for c in B_CUTS] + [B_LONG._replace(model=m) for m in B_LONG_MODELS]
    return [s for s in out if models is None or s.model in models]


@functools.lru_cache(maxsize=None)
def b_build(name, L):
    """E (k,3,L,q) uniform in [0.05, 0.95]: one batch per model and length, cut in every way of B_CUTS."""
    A, _ = model(name)
    rng = np.random.default_rng([22, (B_MODELS + B_LONG_MODELS).index(name), L])
    return _frozen((rng.random((A.shape[0], B, L, A.shape[-1])) * 0.9 + 0.05).astype(np.float32))[0]


@functools.lru_cache(maxsize=None)
def oracle(name, kind, L=None):
    """The unsharded fp64 oracle of a section-B (kind "b") or section-C (kind "c") batch: gamma (k,b,L,q), ll (k,b)."""
    from oracle import textbook
    A, pi = model(name)
    E = b_build(name, L) if kind == "b" else c_build(name)[0]
    res = [textbook.posterior(A[m], pi[m], E[m]) for m in range(A.shape[0])]
    return _frozen(np.stack([g for g, _ in res]), np.stack([ll for _, ll in res]))


# ---- section C ------------------------------------------------------------------------------------------------------
C_L, C_CUTS, C_CHUNK = 96, (0, 32, 64, 96), 16
C_MODELS = ("g15", "g7", "d12")
C_NONPRIMITIVE = ("shipped15", "eye12", "g7absent")          # phi = +inf for every sequence on every rank
RUN_STATE = {"g15": 9, "g7": 4, "d12": 5}                    # g15: EI1, g7: E0 -- both left after one step for certain
RUN_LEN = (1, 2, 4, 8)
PLACEMENTS = ("inside", "before", "after", "straddle")
# kind: "run" | "ends" | "path" | "mark" | "free";  place: a PLACEMENTS entry, or the slab that holds a "mark" pair.
# "mark": two all-zero emission rows at chunk positions (even, odd), even >= 2: the sparse reduce sums its columns after
# position 0 and after every odd position of a chunk, so both rows fall between two sums, the columns lose 2^-106 there
# and the chunk is marked.  "free": zero rows that a sum separates (the first two positions of a chunk; an (odd, even)
# pair; one row on each side of a cut): no column leaves fp32's range, nothing is marked, nothing needs to be.
Hard = collections.namedtuple("Hard", "kind place n pos")


def _run_start(place, n, cut):
    return {"inside": cut + 8, "before": cut - n, "after": cut, "straddle": cut - n // 2}[place]


def c_layout():
    """The hard sequences of one model, in batch order."""
    out = [Hard("run", pl, n, _run_start(pl, n, cut)) for cut in C_CUTS[1:-1] for n in RUN_LEN for pl in PLACEMENTS
           if not (pl == "straddle" and n == 1)]                             # (one position cannot straddle)
    out += [Hard("ends", None, 1, 0), Hard("ends", None, 2, 0)]             # a run at position 0 and one at the end
    out += [Hard("path", None, 0, 20), Hard("path", None, 1, 20)]           # 1e-10 / 1e-20 on the most probable states
    out += [Hard("mark", 0, 2, 10), Hard("mark", 1, 2, 40), Hard("mark", 2, 2, 88)]    # two all-zero rows in a row
    out += [Hard("free", None, 2, 31), Hard("free", None, 2, 80), Hard("free", None, 2, 41)]
    return out


def c_build(name, seed=None):
    return _c_build(name, C_SEED if seed is None else seed)


@functools.lru_cache(maxsize=None)
def _c_build(name, seed):
    """-> E (1,b,96,q) float32, [Hard per sequence].  The non-primitive models get three plain sequences."""
    A, pi = model(name)
    q = A.shape[-1]
    lay = [None] * B if name in C_NONPRIMITIVE else c_layout()
    E = np.empty((1, len(lay), C_L, q), np.float32)
    for s in range(len(lay)):                                # (a stream per sequence: a longer layout moves none)
        rng = np.random.default_rng([23, (C_MODELS + C_NONPRIMITIVE).index(name), seed, s])
        E[0, s] = rng.random((C_L, q)) * 0.9 + 0.05
    if name in C_NONPRIMITIVE:
        return _frozen(E)[0], lay
    st = RUN_STATE[name]

    def run(s, lo, n):
        E[0, s, lo:lo + n] = 0.0
        E[0, s, lo:lo + n, st] = 0.5

    for s, h in enumerate(lay):
        if h.kind == "run":
            run(s, h.pos, h.n)
        elif h.kind == "ends":
            run(s, 0, h.n)
            run(s, C_L - h.n, h.n)
        elif h.kind == "path":
            from oracle import textbook
            g = textbook.posterior(A[0], pi[0], E[0, s:s + 1])[0][0]
            t = np.arange(20, 76)
            E[0, s, t, g[t].argmax(-1)] = 1e-10 if h.n == 0 else 1e-20
        elif h.kind in ("mark", "free"):
            E[0, s, h.pos:h.pos + 2] = 0.0
    return _frozen(E)[0], lay


def verdicts(name, E=None):
    """The reference's summed phi (b,) of a section-C batch (RefBackend over C_CUTS)."""
    A, pi = model(name)
    E = c_build(name)[0] if E is None else E
    _, _, phis = ref_run(A, pi, E, list(C_CUTS))
    return np.sum(phis, axis=0)[0].astype(np.float64)


def certify(name, copies=8):
    """-> (flags (b,) bool, robust (b,) bool): a (case, sequence) pair is robust if the reference's verdict is the same
    on the case and on `copies` copies with every non-zero emission multiplied by 1 + 1e-6 N(0,1), and the summed phi
    stays outside [PHI_LIMIT / 4, 4 PHI_LIMIT] in all of them.  "mark" and "free" sequences are never robust: their
    verdict on the engine comes from the sparse reduce's mark, which the fp64 restatement has no use for."""
    E, lay = c_build(name)
    rng = np.random.default_rng([24, C_MODELS.index(name)])
    runs = [verdicts(name)]
    for _ in range(copies):
        Ep = (E.astype(np.float64) * (1 + 1e-6 * rng.standard_normal(E.shape))).astype(np.float32)
        Ep[E == 0] = 0.0
        runs.append(verdicts(name, Ep))
    phi = np.stack(runs)
    flags = ~(phi <= PHI_LIMIT)
    robust = (flags == flags[0]).all(0) & ~((phi >= PHI_LIMIT / 4) & (phi <= 4 * PHI_LIMIT)).any(0)
    robust &= np.array([h.kind not in ("mark", "free") for h in lay])
    return flags[0], robust


# Seed of the section-C batches: the first of 0, 1, 2, ... that meets the conditions of the CPU test (seed 0 leaves fewer
# than a third of the robust sequences flagged; seed 1: 102 of 120 sequences robust, 35 of them flagged).  ROBUST: per
# model the robust sequences (indices into c_layout()) by verdict, as certify() derives them;
# tests/test_seqshard_sweep_cpu.py re-derives both.
C_SEED = 1
ROBUST = {
    "g15": dict(flagged=(3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 18, 19, 22, 23, 24, 25, 26, 27, 28, 29, 31),
              unflagged=(0, 1, 2, 15, 16, 17, 20, 21, 30, 32, 33)),
    "g7": dict(flagged=(4, 5, 6, 11, 12, 13, 14, 20, 21, 27, 28, 29),
              unflagged=(0, 1, 2, 3, 7, 8, 9, 10, 15, 16, 17, 18, 19, 22, 23, 24, 25, 26, 30, 31, 32, 33)),
    "d12": dict(flagged=(),
              unflagged=(0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32, 33)),
}


# ---- the engine over a list of cuts (GPU tests only) ----------------------------------------------------------------
def sharded_full(A, pi, E, cuts, mode=0, streams=None):
    """A (k,q,q), pi (k,q), E (k,b,L,q) numpy; cuts = slab boundaries: the R slabs through the engine's own
    hmm_seqshard_reduce / hmm_seqshard_posterior one after the other on one GPU, one stream (hence one workspace) per
    "rank".  -> dict(out (k,b,L,q), lls, phis, ops, exs: one entry per rank, numpy)."""
    from hmm_layer_amd import seqshard

    def dev(x):
        return torch.as_tensor(np.array(x, dtype=np.float32, order="C"), device="cuda:0")

    R = len(cuts) - 1
    Ad, pid = dev(A), dev(pi)
    slabs = [dev(E[:, :, cuts[r]:cuts[r + 1]]) for r in range(R)]
    be = seqshard.EngineBackend()
    # one workspace per "rank": the chunk operators of step 1 have to survive until step 3
    streams = streams or [torch.cuda.Stream() for _ in range(R)]
    ops, exs = [], []
    for r in range(R):
        with torch.cuda.stream(streams[r]):
            o, e = be.reduce(Ad, slabs[r], r == 0, R)
        ops.append(o)
        exs.append(e)
    torch.cuda.synchronize()
    all_ops, all_exps = seqshard.stack_slab_operators(ops, exs)
    torch.cuda.synchronize()                    # (stacked on the default stream, consumed on the ranks' streams)
    outs, lls, phis = [], [], []
    for r in range(R):
        with torch.cuda.stream(streams[r]):
            o, ll, ph = be.posterior(Ad, pid, slabs[r], all_ops, all_exps, r, mode)
        streams[r].synchronize()
        outs.append(o.cpu().numpy())
        lls.append(ll.cpu().numpy())
        phis.append(ph.cpu().numpy())
    return dict(out=np.concatenate(outs, axis=2), lls=lls, phis=phis, ops=[o.cpu().numpy() for o in ops],
                exs=[e.cpu().numpy() for e in exs])


def sharded(A, pi, E, cuts, mode=0):
    """-> out, loglik per rank, phi summed over the ranks."""
    res = sharded_full(A, pi, E, cuts, mode)
    return res["out"], res["lls"], np.sum(res["phis"], axis=0)
