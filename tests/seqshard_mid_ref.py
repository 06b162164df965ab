"""fp64 numpy restatement of the two LOCAL steps of the sequence-sharded posterior for 17 to 64 states (test
infrastructure): tests/seqshard_ref.py's RefBackend at width QT = 32 (17..32 states) or 64, with the operator format
and padding of hmm_seqshard_mid_* (include/hmm_engine.h): op[i][k] * 2^exp[k] = the product of the slab's step
matrices, i = state at the slab's last position, k = state just before the slab; rows, columns and exponents from q
on are 0.  All three output modes.  Drives hmm_layer_amd/seqshard.py's exchange on CPU tensors
(tests/test_seqshard_mid_cpu.py) and is what tests/test_seqshard_mid_gpu.py compares the kernels' operators and
verdicts with."""
import numpy as np
import torch

from seqshard_ref import EPS, _rescale


def tile(q):
    return 32 if 17 <= q <= 32 else (64 if 33 <= q <= 64 else 0)


def primitive(A, eps=EPS):
    """The engine's question of a model (k32_check / k64_check): is the support of A (entries > eps) primitive?  S^4096,
    twelve squarings: Wielandt's bound for q = 64 is (q-1)^2 + 1 = 3970."""
    P = np.asarray(A) > eps
    for _ in range(12):
        P = (P.astype(np.int64) @ P.astype(np.int64)) > 0
    return bool(P.all())


class RefBackend:
    def reduce(self, A, E_slab, seq_start, R):
        A, E = A.numpy().astype(np.float64), E_slab.numpy().astype(np.float64)
        k, b, L, q = E.shape
        QT = tile(q)
        op = np.zeros((k, b, QT, QT), np.float32)
        ex = np.zeros((k, b, QT), np.int32)
        At = np.swapaxes(A, 1, 2)[:, None]                   # every sequence of a model at once
        X = np.broadcast_to(np.eye(q), (k, b, q, q)).copy()
        e = np.zeros((k, b, q), np.int64)
        for t in range(L):
            em = np.maximum(E[:, :, t], EPS)
            if t == 0 and seq_start:
                X = em[..., None] * X
            else:
                X = em[..., None] * np.matmul(At, X)
            X, e = _rescale(X, e)
        op[..., :q, :q] = X
        ex[..., :q] = e
        return torch.from_numpy(op), torch.from_numpy(ex)

    def posterior(self, A, pi, E_slab, all_ops, all_exps, r, mode):
        A, E = A.numpy().astype(np.float64), E_slab.numpy().astype(np.float64)
        pi = pi.numpy().astype(np.float64).reshape(A.shape[0], -1)
        ops, exs = all_ops.numpy().astype(np.float64), all_exps.numpy().astype(np.int64)
        k, b, L, q = E.shape
        R = ops.shape[2]
        out = np.zeros((k, b, L, q), np.float32)
        ll = np.zeros((k, b))
        phi = np.zeros((k, b), np.float32)
        prim = [primitive(A[m]) for m in range(k)]
        for m in range(k):
            for s in range(b):
                # (columns relative to the slab's largest exponent: a slab of a thousand positions is beyond fp64's range)
                top = [int(exs[m, s, j, :q].max()) for j in range(R)]
                X = [ops[m, s, j, :q, :q] * np.ldexp(1.0, exs[m, s, j, :q] - top[j])[None, :] for j in range(R)]
                # alpha_hat entering slab r, log-likelihood of the whole sequence
                a, tot = np.maximum(pi[m], EPS), 0.0
                ent = None
                for j in range(R):
                    if j == r:
                        ent = a.copy()
                    a = X[j] @ a
                    tot += np.log(a.sum()) + top[j] * np.log(2.0)
                    a = a / a.sum()
                # beta leaving slab r
                v = np.ones(q)
                for j in range(R - 1, r, -1):
                    v = X[j].T @ v
                    v = v / v.max()
                # serial cell recursion on the slab
                ah = np.zeros((L, q))
                fm = np.zeros((L, q), bool)                              # forward prediction sat at the clamp
                x = ent
                for t in range(L):
                    em = np.maximum(E[m, s, t], EPS)
                    first = t == 0 and r == 0
                    pred = x if first else x @ A[m]
                    fm[t] = (pred <= EPS) & (not first)
                    sf = em * np.maximum(pred, EPS)
                    x = sf / sf.sum()
                    ah[t] = x
                Rv, acc = v, 0.0
                bm = np.zeros(q, bool)
                g = np.zeros((L, q))
                for t in range(L - 1, -1, -1):
                    gt = ah[t] * Rv
                    gt = gt / gt.sum()
                    acc += gt[fm[t]].sum() + gt[bm].sum()                # psi: posterior mass on clamp-born components
                    g[t] = gt
                    bh = np.maximum(E[m, s, t], EPS) * Rv
                    u = A[m] @ (bh / bh.sum())
                    bm = u <= EPS
                    Rv = np.maximum(u, EPS)
                with np.errstate(divide="ignore"):
                    out[m, s] = g if mode == 0 else (np.log(g) if mode == 1 else np.log(g) + tot)
                ll[m, s] = tot
                phi[m, s] = acc if prim[m] else np.inf
        return torch.from_numpy(out), torch.from_numpy(ll), torch.from_numpy(phi)

    def unsharded(self, A, pi, E, mode):
        """The unsharded call of gather_flagged: the serial fp64 recursion with the cell's clamps."""
        from oracle import textbook
        g, ll = textbook.posterior(A[0].numpy(), pi[0].numpy(), E[0].numpy())
        with np.errstate(divide="ignore"):
            o = g if mode == 0 else (np.log(g) if mode == 1 else np.log(g) + ll[:, None, None])
        return torch.from_numpy(o.astype(np.float32))[None], torch.from_numpy(ll)[None]
