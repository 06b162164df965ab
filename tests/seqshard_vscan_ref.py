"""The sequence-sharded Viterbi protocol for up to 64 states (include/hmm_engine.h: hmm_seqshard_vscan_*) restated in
int64 numpy: tests/seqshard_viterbi_ref.py's formulas at width QT = 32 (q <= 32) or 64, with the padding the header
states (-2^30 in the rows and columns of an operator from q on, 0 in the bases and maps).

Test infrastructure; imports neither the engine nor a GPU.  RefVscanBackend has the three methods of
seqshard.ViterbiEngineBackend, so seqshard.viterbi runs on it over gloo and run_cuts() plays a list of cuts on it.
"""
import numpy as np
import torch

from seqshard_viterbi_ref import KINDS, _hop, _np, build, oracle_run, run_cuts  # noqa: F401  (shared, unchanged)
from oracle.viterbi import FRAC_BITS, quantise

VS_NEG = -(1 << 30)


def tile(q):
    return 32 if q <= 32 else 64


def slab_operators(logA, logpi, logE, seq_start, lengths):
    """The operators of the slabs logE[:, :, :Ls] for every Ls of `lengths` (increasing), from one pass over the longest:
    -> [(vop (k,b,QT,QT) int32, vbase (k,b,QT) int64) per length], torch CPU tensors."""
    a, p0, e = quantise(_np(logA)), quantise(_np(logpi)), quantise(_np(logE))
    k, b, _, q = e.shape
    QT = tile(q)
    a = a.reshape(k, 1, q, q)
    if seq_start:                                            # every column: the scores after position 0 from pi
        X = (p0.reshape(k, 1, q) + e[:, :, 0])[..., None]    # (one column: the recursion is the same in all of them)
    else:                                                    # X[j][i]: from state i before the slab into j at its position 0
        X = np.broadcast_to(np.swapaxes(a, -1, -2) + e[:, :, 0][..., None], (k, b, q, q)).copy()
    out = []
    for t in range(1, max(lengths) + 1):
        if t in lengths:
            Xf = np.broadcast_to(X, (k, b, q, q))
            base = Xf.max(-2)                                # per column i
            vop = np.full((k, b, QT, QT), VS_NEG, np.int32)
            vbase = np.zeros((k, b, QT), np.int64)
            vop[..., :q, :q] = Xf - base[..., None, :]
            vbase[..., :q] = base
            out.append((torch.from_numpy(vop), torch.from_numpy(vbase)))
        if t < max(lengths):
            # X'[j][i] = max_m(X[m][i] + a[m][j]) + e_t[j]
            X = (X[:, :, :, None, :] + a[:, :, :, :, None]).max(2) + e[:, :, t][..., None]
    assert len(out) == len(lengths) and list(lengths) == sorted(lengths)
    return out


class RefVscanBackend:
    """One instance per rank: apply() keeps the slab's backpointers for path(), as the engine's workspace does."""

    def reduce(self, logA, logpi, logE_slab, seq_start, R):
        return slab_operators(logA, logpi, logE_slab, seq_start, [_np(logE_slab).shape[2]])[0]

    def apply(self, logA, logpi, logE_slab, all_vops, all_vbases, r):
        a, p0, e = quantise(_np(logA)), quantise(_np(logpi)), quantise(_np(logE_slab))
        k, b, Ls, q = e.shape
        QT = tile(q)
        a = a.reshape(k, 1, q, q)
        vops, vbases = _np(all_vops).astype(np.int64), _np(all_vbases).astype(np.int64)
        R = vops.shape[2]
        assert vops.shape == (k, b, R, QT, QT) and vbases.shape == (k, b, R, QT)
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
        origin = np.zeros((k, b, QT), np.uint8)
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
        assert org.shape == (k, b, R, tile(q))
        s = _np(final_state).astype(np.int64)[..., None]     # (k,b,1)
        for c in range(R - 1, r, -1):
            s = np.take_along_axis(org[:, :, c], s, -1)
        path = np.zeros((k, b, Ls), np.int32)
        for t in range(Ls - 1, -1, -1):
            path[:, :, t] = s[..., 0]
            if t > 0:
                s = np.take_along_axis(self._bp[:, :, t], s, -1)
        return torch.from_numpy(path)
