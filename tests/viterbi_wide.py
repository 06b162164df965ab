"""A numpy restatement of the Viterbi definition (oracle/viterbi.py) for any number of states.

The oracles keep backpointers as int8, so above 127 states they cannot check hmm_viterbi_large; this
restatement keeps int64 scores and int32 backpointers and is otherwise the same serial recursion:
    d_0[j] = Q(log pi[j]) + Q(log E_0[j]),  d_t[j] = max_i (d_{t-1}[i] + Q(log A[i,j])) + Q(log E_t[j]),
lowest maximising index in the recursion and at the final state, score = d_{L-1} / 2**16."""
import numpy as np

from oracle.viterbi import FRAC_BITS, quantise


def viterbi(logA, logpi, logE, chunk=1 << 22):
    """logA (q,q), logpi (q,), logE (b,L,q) or (L,q) fp32 -> path (b,L) int32, score (b,) float64.
    Candidates are formed for as many sequences at once as `chunk` int64 entries allow."""
    a = quantise(logA)
    p0 = quantise(logpi).reshape(-1)
    e = quantise(logE)
    if e.ndim == 2:
        e = e[None]
    b, L, q = e.shape
    path = np.zeros((b, L), dtype=np.int32)
    score = np.zeros(b, dtype=np.float64)
    step = max(1, chunk // (q * q))
    for s0 in range(0, b, step):
        es = e[s0:s0 + step]
        n = es.shape[0]
        bp = np.zeros((n, L, q), dtype=np.int32)
        d = p0[None, :] + es[:, 0]
        for t in range(1, L):
            cand = d[:, :, None] + a[None, :, :]            # (n, i, j)
            bp[:, t] = cand.argmax(axis=1)                  # first (lowest) maximiser
            d = cand.max(axis=1) + es[:, t]
        s = d.argmax(axis=1)
        score[s0:s0 + n] = d[np.arange(n), s].astype(np.float64) / (1 << FRAC_BITS)
        for t in range(L - 1, -1, -1):
            path[s0:s0 + n, t] = s
            if t > 0:
                s = bp[np.arange(n), t, s]
    return path, score


def random_model(rng, q, kind):
    """fp32 (logA, logpi) test models: 'dense' (every edge), 'band' (profile-like: a band of likely edges
    over a floor), 'sparse' (a few random predecessors per state, every other edge -inf)."""
    if kind == "dense":
        A = rng.random((q, q)).astype(np.float32) + np.float32(0.01)
    elif kind == "band":
        A = rng.random((q, q)).astype(np.float32) ** 8
        A *= (np.abs(np.subtract.outer(np.arange(q), np.arange(q))) < 40) + 1e-4
    elif kind == "sparse":
        A = np.zeros((q, q), dtype=np.float32)
        for j in range(q):
            deg = 1 + int(rng.integers(0, min(q, 6)))
            A[rng.choice(q, deg, replace=False), j] = rng.random(deg) + 0.05
        A[np.arange(q), rng.integers(0, q, q)] += 0.05     # no state without a successor
    else:
        raise ValueError(kind)
    A /= A.sum(-1, keepdims=True)
    pi = rng.random(q).astype(np.float32) + np.float32(0.01)
    with np.errstate(divide="ignore"):
        return np.log(A).astype(np.float32), np.log(pi / pi.sum()).astype(np.float32)


def random_logE(rng, b, L, q, dead=0.05):
    logE = (-6 * rng.random((b, L, q))).astype(np.float32)
    logE[rng.random(logE.shape) < dead] = -np.inf
    return logE
