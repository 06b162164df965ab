"""Models, inputs, norms and drivers of the tests of the sequence-sharded posterior for 17 to 64 states
(hmm_seqshard_mid_reduce / hmm_seqshard_mid_posterior, csrc/hmm_seqshard_mid.inc, driven by hmm_layer_amd/seqshard.py
through hmm_layer_amd/seqshard_mid.py).

Test infrastructure; imports neither the engine library nor a GPU at module level (the engine drivers import them when
called).  tests/test_seqshard_mid_cpu.py proves from the fp64 restatement (tests/seqshard_mid_ref.py) and the oracle
alone that these inputs can carry the comparison; tests/test_seqshard_mid_gpu.py runs the kernels on them.

Models (model(name) -> A (k,q,q), pi (k,q) float32, read-only):
  "g29" "g43" "g57"   the two- to four-copy gene models, GenePredMultiHMMTransitioner(k = 2, 3, 4; 200, 4500, 10000)
  "d17" .. "d64"      dense random models (rand_model of tests/seqshard_cases.py), one per state count
  "g29+d29"           two models in one call (sparse waves straddling two models)
  "eye20", "red29"    models whose support is not primitive: the identity; a 29-state matrix that cannot leave its
                      last five states (reducible)
"""
import collections
import functools
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch

import seqshard_cases as sc
from seqshard_cases import PHI_LIMIT, GAMMA_TOL, LL_REL, LL_ABS, NO_LL_REL, TOL_FLOOR, TOL_FACTOR, op_error, _frozen
from seqshard_mid_ref import RefBackend, tile

EPS = 1e-16
B = 3
GENE = ("g29", "g43", "g57")
DENSE = ("d17", "d24", "d32", "d33", "d48", "d64")
TWO = ("g29+d29",)
MODELS = GENE + DENSE + TWO
NONPRIMITIVE = ("eye20", "red29")


@functools.lru_cache(maxsize=None)
def _single(name):
    q = int(name[-2:])
    if name[0] == "g":
        import postgrad_mid_cases as pm
        A, pi = pm.gene_model((q - 1) // 14)
        return _frozen(np.array(A), np.array(pi))
    if name == "eye20":
        return _frozen(np.eye(20, dtype=np.float32), np.full(20, 1 / 20, dtype=np.float32))
    if name == "red29":
        A, pi = sc.rand_model(np.random.default_rng([12, 29]), 29)
        A = A.copy()
        A[24:, :24] = 0.0                                    # nothing leaves the last five states
        A /= A.sum(-1, keepdims=True)
        return _frozen(A.astype(np.float32), pi)
    assert name[0] == "d", name
    return _frozen(*sc.rand_model(np.random.default_rng([11, q]), q))


@functools.lru_cache(maxsize=None)
def model(name):
    Ms = [_single(n) for n in name.split("+")]
    return _frozen(np.stack([m[0] for m in Ms]), np.stack([m[1] for m in Ms]))


# ---- the fp64 restatement over a list of cuts, and its fp32 twin of the reduce ------------------------------------
def ref_run(A, pi, E, cuts, mode=0):
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
        o, ll, ph = be.posterior(At, pit, slabs[r], ops, exs, r, mode)
        outs.append(o.numpy())
        lls.append(ll.numpy())
        phis.append(ph.numpy())
    return np.concatenate(outs, axis=2), lls, phis


def op32(A, E_slab, seq_start):
    """The slab operator formed step by step in float32 numpy (tests/seqshard_cases.py::op32 at width QT)."""
    A, E = np.asarray(A, np.float32), np.asarray(E_slab, np.float32)
    k, b, L, q = E.shape
    At = np.ascontiguousarray(np.swapaxes(A, 1, 2))[:, None]
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
    QT = tile(q)
    op = np.zeros((k, b, QT, QT), np.float32)
    ex = np.zeros((k, b, QT), np.int32)
    op[..., :q, :q] = X
    ex[..., :q] = e
    return op, ex


# ---- section A: the slab operator -----------------------------------------------------------------------------------
ASpec = collections.namedtuple("ASpec", "model Ls seq_start variant chunk dense")
SHORT_LS = (1, 2, 16, 17, 100)
LONG_LS = (496, 512, 513, 1000)                              # OPT_CHUNK = 16: 31, 32, 33, 63 chunks
LONG_MODELS = ("g29", "d33")
VARIANTS = ("plain", "dead", "tiny")


def a_id(s):
    return "%s-Ls%d-start%d-%s-chunk%d-dense%d" % s


def a_cases():
    """Every model at the short lengths, plain; the variants and both seq_start on one model per reduce kernel and
    width (g29 sparse and dense, d32, d64: no pad lane, g29+d29); the long slabs (both sides of the two-level compose)
    on one model per width."""
    out = [ASpec(m, Ls, ss, "plain", 16, 0) for m in MODELS for Ls in SHORT_LS for ss in (0, 1)]
    out += [ASpec("g29", Ls, ss, "plain", 16, 1) for Ls in SHORT_LS for ss in (0, 1)]
    out += [ASpec(m, Ls, ss, v, 16, d) for m, d in (("g29", 0), ("g29", 1), ("d32", 0), ("d64", 0), ("g29+d29", 0))
            for Ls in (17, 100) for ss in (0, 1) for v in ("dead", "tiny")]
    out += [ASpec(m, Ls, ss, v, 16, 0) for m in LONG_MODELS for Ls in LONG_LS for ss in (0, 1)
            for v in (("plain", "tiny") if Ls == 1000 else ("plain",))]
    return out


@functools.lru_cache(maxsize=None)
def a_build(spec):
    """E (k,3,Ls,q): uniform in [0.05, 0.95]; "dead": state q // 2 emits exact zeros throughout; "tiny": every emission
    is scaled by 1e-10 and three states emit 1e-10 flat (tests/seqshard_cases.py::_a_build)."""
    A, _ = model(spec.model)
    k, q = A.shape[:2]
    rng = np.random.default_rng([31, MODELS.index(spec.model), spec.Ls, spec.seq_start, VARIANTS.index(spec.variant)])
    E = (rng.random((k, B, spec.Ls, q)) * 0.9 + 0.05).astype(np.float32)
    if spec.variant == "dead":
        E[..., q // 2] = 0.0
    elif spec.variant == "tiny":
        E *= np.float32(1e-10)
        E[..., sc.tiny_states(q)] = 1e-10
    return _frozen(E)[0]


@functools.lru_cache(maxsize=None)
def a_reference(spec):
    """-> dict(op, ex: RefBackend.reduce; e32: op32's error against it; limit = max(4 e32, 1e-6)).  The dense flag
    changes the kernel, not the reference."""
    spec = spec._replace(dense=0)
    return _a_reference(spec)


@functools.lru_cache(maxsize=None)
def _a_reference(spec):
    A, _ = model(spec.model)
    E = a_build(spec)
    op, ex = RefBackend().reduce(torch.from_numpy(np.array(A)), torch.from_numpy(np.array(E)), spec.seq_start, 1)
    op, ex = op.numpy(), ex.numpy()
    o32, x32 = op32(A, E, spec.seq_start)
    e32 = op_error(o32, x32, op, ex, A.shape[-1])
    return dict(op=op, ex=ex, e32=e32, limit=max(TOL_FACTOR * e32, TOL_FLOOR))


# ---- section B: benign batches --------------------------------------------------------------------------------------
B_L = 203
B_CUTS = ((0, B_L), (0, 1, B_L), (0, 100, 101, B_L), (0, 50, 120, 202, B_L),
          tuple(range(0, B_L, 26))[:8] + (B_L,))             # ... and eight slabs: seven of 26 positions, one of 21
B_LONG_L, B_LONG_CUTS = 1513, (0, 513, 1513)                 # 33 and 63 chunks of 16: both slabs compose in two levels
B_LONG_MODELS = ("g29", "d33")


@functools.lru_cache(maxsize=None)
def b_build(name, L):
    """E (k,3,L,q) uniform in [0.05, 0.95]: one batch per model and length, cut in every way of B_CUTS."""
    A, _ = model(name)
    rng = np.random.default_rng([32, (MODELS + NONPRIMITIVE).index(name), L])
    return _frozen((rng.random((A.shape[0], B, L, A.shape[-1])) * 0.9 + 0.05).astype(np.float32))[0]


@functools.lru_cache(maxsize=None)
def oracle(name, L):
    """The unsharded fp64 oracle of a section-B batch: gamma (k,b,L,q), ll (k,b)."""
    from oracle import textbook
    A, pi = model(name)
    E = b_build(name, L)
    res = [textbook.posterior(A[m], pi[m], E[m]) for m in range(A.shape[0])]
    return _frozen(np.stack([g for g, _ in res]), np.stack([ll for _, ll in res]))


# ---- section C: hard inputs -----------------------------------------------------------------------------------------
C_L, C_RUN = 120, (50, 70)
# cuts: none; clear of the run; across it; the run starts at a cut and ends at the next
G43_CUTS = ((0, 120), (0, 40, 80, 120), (0, 60, 120), (0, 50, 70, 120))
# (model, the state that alone emits during the run, cuts).  All three states are first-exon-phase states that are left
# after one step for certain, so the run is survived at the floor only.  Whether the restatement flags the sequence
# depends on the copy: on these emissions it does for state 8 of g29 and state 11 of g43 (summed phi 0.41 .. 0.83 and
# 0.24 .. 0.49) and does not for state 10 of g43 (phi 7e-14, the result as accurate as a benign one: every path
# survives the floor equally, which is linear) -- as for state 7 of g29, which is not used.
C_CASES = (("g29", 8, (0, 60, 120)),) + tuple(("g43", st, c) for st in (10, 11) for c in G43_CUTS)
C_FLAGGED = {("g29", 8): True, ("g43", 10): False, ("g43", 11): True}


def c_id(v):
    return v if isinstance(v, str) else (str(v) if isinstance(v, int) else "_".join(map(str, v)))


@functools.lru_cache(maxsize=None)
def c_build(name, state):
    """E (1,3,120,q): sequence 1 emits from `state` alone (0.5, all others 0) at positions 50 .. 69."""
    A, _ = model(name)
    q = A.shape[-1]
    rng = np.random.default_rng([33, q])
    E = (rng.random((1, B, C_L, q)) * 0.9 + 0.05).astype(np.float32)
    E[0, 1, C_RUN[0]:C_RUN[1]] = 0.0
    E[0, 1, C_RUN[0]:C_RUN[1], state] = 0.5
    return _frozen(E)[0]


@functools.lru_cache(maxsize=None)
def c_oracle(name, state):
    from oracle import textbook
    A, pi = model(name)
    g, ll = textbook.posterior(A[0], pi[0], c_build(name, state)[0])
    return _frozen(g[None], ll[None])


@functools.lru_cache(maxsize=None)
def c_reference(name, state, cuts):
    """The restatement on a hard case: out, the summed phi (3,), the flags."""
    A, pi = model(name)
    out, _, phis = ref_run(A, pi, c_build(name, state), list(cuts))
    phi = np.sum(phis, axis=0)[0].astype(np.float64)
    return out, phi, ~(phi <= PHI_LIMIT)


# ---- the engine over a list of cuts (GPU tests only) ----------------------------------------------------------------
def dev(x, dtype=np.float32):
    return torch.as_tensor(np.array(x, dtype=dtype, order="C"), device="cuda:0")


def sharded_full(A, pi, E, cuts, mode=0, streams=None):
    """A (k,q,q), pi (k,q), E (k,b,L,q) numpy; cuts = slab boundaries: the R slabs through hmm_seqshard_mid_reduce /
    hmm_seqshard_mid_posterior one after the other on one GPU, one stream (hence one workspace) per "rank".
    -> dict(out (k,b,L,q), lls, phis, ops, exs: one entry per rank, numpy)."""
    from hmm_layer_amd import seqshard
    R = len(cuts) - 1
    Ad, pid = dev(A), dev(pi)
    slabs = [dev(E[:, :, cuts[r]:cuts[r + 1]]) for r in range(R)]
    be = seqshard.posterior_backend(int(E.shape[-1]))
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


class FakeGroup:
    """torch.distributed's calls as seqshard.posterior and seqshard.gather_flagged make them, answered in place for a
    group of R ranks that are played one after the other in one process (no process group), one model per call.
    Pass 1 (recording = True, seqshard.posterior alone) records what each rank contributes: its slab operators and its
    certificate.  Pass 2 hands every rank the others' contributions.  gather_flagged (root 0): rank 0 is played first
    and "receives" the other ranks' slabs of the flagged sequences (flag_seqs, set by the test from pass 1) from
    `slabs`; what it sends and broadcasts is kept for the ranks played after it."""

    def __init__(self, slabs):
        self.slabs, self.R = slabs, len(slabs)
        self.gathered = collections.defaultdict(dict)        # call index -> {rank: tensor}
        self.reduced = collections.defaultdict(dict)
        self.sent, self.bcast, self.flag_seqs = {}, [], []
        self.play(0, True)

    def install(self, monkeypatch):
        import torch.distributed as dist
        monkeypatch.setattr(dist, "get_world_size", lambda group=None: self.R)
        monkeypatch.setattr(dist, "get_rank", lambda group=None: self.rank)
        for name in ("all_gather", "all_reduce", "send", "recv", "broadcast"):
            monkeypatch.setattr(dist, name, getattr(self, name))

    def play(self, rank, recording):
        self.rank, self.recording, self.calls, self.nb = rank, recording, 0, 0

    def all_gather(self, outs, x, group=None):
        if x.dtype == torch.int64 and x.numel() == 1:        # gather_flagged's slab lengths
            for r in range(self.R):
                outs[r].fill_(self.slabs[r].shape[2])
            return
        i, self.calls = self.calls, self.calls + 1
        if self.recording:
            self.gathered[i][self.rank] = x.clone()
        for r in range(self.R):
            outs[r].copy_(x if self.recording else self.gathered[i][r])

    def all_reduce(self, x, op=None, group=None):
        i, self.calls = self.calls, self.calls + 1
        if self.recording:
            self.reduced[i][self.rank] = x.clone()
        else:
            x.copy_(sum(self.reduced[i][r] for r in range(self.R)))

    def send(self, x, dst=None, group=None):
        self.sent.setdefault((self.rank, dst), []).append(x.clone())

    def recv(self, buf, src=None, group=None):
        if self.rank == 0:                                   # the root: rank src's slab of the flagged sequences
            buf.copy_(self.slabs[src][0, torch.as_tensor(self.flag_seqs, device=buf.device)])
        else:
            buf.copy_(self.sent[(src, self.rank)].pop(0))

    def broadcast(self, x, src=None, group=None):
        if self.rank == src:
            self.bcast.append(x.clone())
        else:
            x.copy_(self.bcast[self.nb])
            self.nb += 1
