"""The sequence-sharded Viterbi protocol (include/hmm_engine.h: hmm_seqshard_viterbi_*) restated in int64 numpy.

Test infrastructure: the restatement the protocol is specified by.  Imports neither the engine nor a GPU.
RefViterbiBackend has the three methods of seqshard.ViterbiEngineBackend (torch CPU tensors or numpy arrays in, torch
CPU tensors out), so seqshard.viterbi runs on it over gloo; run_cuts() plays the ranks of a list of cuts in turn on any
backend; build() makes the inputs both test files share.

Semantics are oracle/viterbi.py's: Q(x) = rint(clip(x, -1024, 1024) * 2^16), d_t[j] = max_i(d_{t-1}[i] + Q(log A[i,j]))
+ Q(log E_t[j]), lowest-index tie-breaks.
"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch

from oracle.viterbi import FRAC_BITS, quantise

QP = 16


def _np(x):
    return x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def _hop(V, d):
    """d'[j] = max_i(V[j][i] + d[i]) over the trailing axes: V (k,b,q,q) [j][i], d (k,b,q)."""
    return (V + d[..., None, :]).max(-1)


class RefViterbiBackend:
    """One instance per rank: apply() keeps the slab's backpointers for path(), as the engine's workspace does."""

    def reduce(self, logA, logpi, logE_slab, seq_start, R):
        a, p0, e = quantise(_np(logA)), quantise(_np(logpi)), quantise(_np(logE_slab))
        k, b, Ls, q = e.shape
        a = a.reshape(k, 1, q, q)
        if seq_start:                                        # every column: the scores after position 0 from pi
            X = np.broadcast_to((p0.reshape(k, 1, q) + e[:, :, 0])[..., None], (k, b, q, q)).copy()
        else:                                                # X[j][i]: from state i before the slab into j at its position 0
            X = np.swapaxes(a, -1, -2) + e[:, :, 0][..., None]
            X = np.broadcast_to(X, (k, b, q, q)).copy()
        for t in range(1, Ls):
            # X'[j][i] = max_m(X[m][i] + a[m][j]) + e_t[j]
            X = (X[:, :, :, None, :] + a[:, :, :, :, None]).max(2) + e[:, :, t][..., None]
        base = X.max(-2)                                     # per column i
        vop = np.zeros((k, b, QP, QP), np.int32)
        vbase = np.zeros((k, b, QP), np.int64)
        vop[..., :q, :q] = X - base[..., None, :]
        vbase[..., :q] = base
        return torch.from_numpy(vop), torch.from_numpy(vbase)

    def apply(self, logA, logpi, logE_slab, all_vops, all_vbases, r):
        a, p0, e = quantise(_np(logA)), quantise(_np(logpi)), quantise(_np(logE_slab))
        k, b, Ls, q = e.shape
        a = a.reshape(k, 1, q, q)
        vops, vbases = _np(all_vops).astype(np.int64), _np(all_vbases).astype(np.int64)
        R = vops.shape[2]
        V = vops[..., :q, :q] + vbases[..., None, :q]        # (k,b,R,q,q) [j][i]
        d = V[:, :, 0, :, 0]                                 # column 0 of operator 0
        enter = None
        for c in range(1, R):
            if c == r:
                enter = d
            d = _hop(V[:, :, c], d)
        final_state = d.argmax(-1).astype(np.int32)          # lowest index among the best
        score = d.max(-1).astype(np.float64) / (1 << FRAC_BITS)
        bp = np.zeros((k, b, Ls, q), np.int64)
        if r == 0:
            x = p0.reshape(k, 1, q) + e[:, :, 0]
        else:
            cand = enter[..., :, None] + a                   # (k,b,i,j)
            bp[:, :, 0] = cand.argmax(-2)
            x = cand.max(-2) + e[:, :, 0]
        for t in range(1, Ls):
            cand = x[..., :, None] + a
            bp[:, :, t] = cand.argmax(-2)
            x = cand.max(-2) + e[:, :, t]
        self._bp = bp
        origin = np.zeros((k, b, QP), np.uint8)
        if r > 0:
            s = np.broadcast_to(np.arange(q), (k, b, q)).copy()
            for t in range(Ls - 1, -1, -1):
                s = np.take_along_axis(bp[:, :, t], s, -1)
            origin[..., :q] = s
        return torch.from_numpy(origin), torch.from_numpy(final_state), torch.from_numpy(score)

    def path(self, dims, all_origins, final_state, r):
        k, b, Ls, q = (int(v) for v in dims)
        org = _np(all_origins).astype(np.int64)
        R = org.shape[2]
        s = _np(final_state).astype(np.int64)[..., None]     # (k,b,1)
        for c in range(R - 1, r, -1):
            s = np.take_along_axis(org[:, :, c], s, -1)
        path = np.zeros((k, b, Ls), np.int32)
        for t in range(Ls - 1, -1, -1):
            path[:, :, t] = s[..., 0]
            if t > 0:
                s = np.take_along_axis(self._bp[:, :, t], s, -1)
        return torch.from_numpy(path)


def run_cuts(make_backend, logA, logpi, logE, cuts, dev=torch.as_tensor, sync=lambda: None):
    """The protocol over the slabs logE[:, :, cuts[r]:cuts[r+1]], ranks played in turn: ALL reduces, then ALL applies,
    then ALL paths (whatever a backend keeps between its calls has to survive the other ranks' calls).
    make_backend(r) -> (backend, context manager under which rank r's calls run); dev puts an array where the backend
    wants it, sync() is called between the phases (ranks on streams of their own).
    -> dict(path (k,b,L) int32, scores / finals: one (k,b) array per rank, vops, vbases, origins: per rank), numpy."""
    R = len(cuts) - 1
    ranks = [make_backend(r) for r in range(R)]
    A, pi = dev(np.array(logA)), dev(np.array(logpi))        # (copies: the inputs may be read-only)
    slabs = [dev(np.array(logE[:, :, cuts[r]:cuts[r + 1]])) for r in range(R)]
    sync()
    red = []
    for r, (be, ctx) in enumerate(ranks):
        with ctx:
            red.append(be.reduce(A, pi, slabs[r], r == 0, R))
    sync()
    all_vops = dev(torch.stack([v.cpu() for v, _ in red], dim=2).contiguous())
    all_vbases = dev(torch.stack([v.cpu() for _, v in red], dim=2).contiguous())
    sync()
    app = []
    for r, (be, ctx) in enumerate(ranks):
        with ctx:
            app.append(be.apply(A, pi, slabs[r], all_vops, all_vbases, r))
    sync()
    all_origins = dev(torch.stack([o.cpu() for o, _, _ in app], dim=2).contiguous())
    sync()
    paths = []
    for r, (be, ctx) in enumerate(ranks):
        with ctx:
            paths.append(be.path(tuple(slabs[r].shape), all_origins, app[r][1], r))
    sync()
    paths = [x.cpu().numpy() for x in paths]
    return dict(path=np.concatenate(paths, axis=2), scores=[s.cpu().numpy() for _, _, s in app],
                finals=[f.cpu().numpy() for _, f, _ in app], vops=[v.cpu().numpy() for v, _ in red],
                vbases=[v.cpu().numpy() for _, v in red], origins=[o.cpu().numpy() for o, _, _ in app])


def oracle_run(logA, logpi, logE):
    """oracle.viterbi model by model: path (k,b,L) int32, score (k,b) float64."""
    from oracle import viterbi as ov
    res = [ov.viterbi(logA[m], logpi[m], logE[m]) for m in range(logE.shape[0])]
    return np.stack([p for p, _ in res]), np.stack([s for _, s in res])


KINDS = ("random", "ties", "flat", "absent")


def build(kind, k, b, L, q, seed=0):
    """-> logA (k,q,q), logpi (k,q), logE (k,b,L,q) float32.
    random: logs of a random stochastic model and of uniform emissions; ties: every log drawn from {0, -1, -2};
    flat: everything -1.5 (the path is all zeros); absent: random with 60 % of log A at -inf."""
    rng = np.random.default_rng([31, KINDS.index(kind), k, b, L, q, seed])
    if kind == "ties":
        draw = lambda *s: -rng.integers(0, 3, s).astype(np.float32)
        return draw(k, q, q), draw(k, q), draw(k, b, L, q)
    if kind == "flat":
        f = lambda *s: np.full(s, -1.5, np.float32)
        return f(k, q, q), f(k, q), f(k, b, L, q)
    A = rng.random((k, q, q)) ** 3 + 1e-3
    A /= A.sum(-1, keepdims=True)
    pi = rng.random((k, q)) + 0.1
    pi /= pi.sum(-1, keepdims=True)
    with np.errstate(divide="ignore"):
        logA = np.log(A).astype(np.float32)
        if kind == "absent":
            logA[rng.random((k, q, q)) < 0.6] = -np.inf
    return logA, np.log(pi).astype(np.float32), np.log(rng.random((k, b, L, q)) * 0.9 + 0.05).astype(np.float32)
