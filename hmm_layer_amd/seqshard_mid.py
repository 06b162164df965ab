"""Sequence-sharded state posteriors for 17 to 64 states: the ctypes binding of hmm_seqshard_mid_* (include/hmm_engine.h).

The protocol is seqshard.posterior's (reduce, all-gather, posterior, all-reduce of the certificate) on the chunked scan
that serves engine.posterior in this range, with q x q operators in tiles of QT = tile(q) = 32 or 64 states;
seqshard.posterior picks this backend for 17 to 64 states.  The symbols are typed here, on the handle engine.lib()
returns, and keep a signature table of their own (SIGNATURES); everything else — device checks, the workspace cache,
the stream, error codes — is engine's.  No CPU compute.
"""
import torch

from . import engine
from .engine import _F, _I, _P, _SZ

# symbol -> (restype, argtypes)
SIGNATURES = {
    "hmm_seqshard_mid_max_states": (_I, []),
    "hmm_seqshard_mid_tile": (_I, [_I]),
    "hmm_seqshard_mid_workspace_bytes": (_SZ, [_I] * 5),
    "hmm_seqshard_mid_reduce": (_I, [_P, _P, _I, _I, _I, _I, _F, _I, _I, _P, _P, _P, _SZ, _P]),
    "hmm_seqshard_mid_posterior": (_I, [_P, _P, _P, _I, _I, _I, _I, _F, _I, _P, _P, _I, _I, _I, _P, _P, _P, _P, _SZ, _P]),
}
WORKSPACE_TAG = "seqshard_mid"
MIN_STATES = 17         # up to 16 states: engine.seqshard_reduce / engine.seqshard_posterior
_typed = None           # the library handle whose symbols have been typed


def lib():
    """engine.lib() with this module's symbols typed.  Raises if the library does not export them."""
    global _typed
    L = engine.lib()
    if _typed is not L:
        for name, (restype, argtypes) in SIGNATURES.items():
            if not hasattr(L, name):
                raise engine.EngineError("the engine library %s does not export %s: rebuild it with "
                                         "`python -m hmm_layer_amd.build`" % (engine.LIB_PATH, name))
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
        _typed = L
    return L


def max_states():
    return lib().hmm_seqshard_mid_max_states()


def tile(q):
    """Edge of the exchanged operators: 32 for 17 to 32 states, 64 for 33 to 64; 0 outside 17 .. 64."""
    return lib().hmm_seqshard_mid_tile(int(q))


def _shapes(A, E, pi=None):
    """engine._shapes without its limit of 16 states: A (k,q,q), pi (k,q), dims = (k, b, Ls, q)."""
    if E.dim() != 4:
        raise ValueError("E_slab must have shape (k, b, Ls, q), got %s" % (tuple(E.shape),))
    k, b, L, q = E.shape
    if A.dim() == 2:
        A = A.unsqueeze(0)
    if tuple(A.shape) != (k, q, q):
        raise ValueError("A must have shape (k=%d, q=%d, q=%d), got %s" % (k, q, q, tuple(A.shape)))
    if pi is not None:
        if pi.numel() != k * q:
            raise ValueError("pi must hold k*q = %d values, got %s" % (k * q, tuple(pi.shape)))
        pi = pi.reshape(k, q)
    if min(k, b, L, q) < 1:
        raise ValueError("empty input: (k, b, Ls, q) = %s" % ((k, b, L, q),))
    if not MIN_STATES <= q <= max_states():
        raise ValueError("hmm_seqshard_mid_* cover %d <= q <= %d states, got %d" % (MIN_STATES, max_states(), q))
    return A, pi, (k, b, L, q)


def _ws(dims, R, device):
    need = lib().hmm_seqshard_mid_workspace_bytes(*dims, int(R))
    if need == 0:
        raise ValueError("bad sequence-sharded posterior call: (k, b, Ls, q) = %s, R = %d" % (tuple(dims), R))
    return engine._workspace(device, need, WORKSPACE_TAG)


def reduce(A, E_slab, seq_start, R, eps=engine.EPS):
    """Step 1: this rank's time slab E_slab (k,b,Ls,q) -> its operator per sequence, slab_op (k,b,QT,QT) fp32 and
    slab_exp (k,b,QT) int32 column exponents (zeros from q on).  The chunk operators stay in this device's
    "seqshard_mid" workspace (one per stream) for posterior()."""
    A, E = engine._dev(A, "A"), engine._dev(E_slab, "E_slab")
    A, _, dims = _shapes(A, E)
    k, b, _, q = dims
    with torch.cuda.device(E.device):
        ws = _ws(dims, R, E.device)
        QT = tile(q)
        op = torch.empty((k, b, QT, QT), dtype=torch.float32, device=E.device)
        ex = torch.empty((k, b, QT), dtype=torch.int32, device=E.device)
        engine._check(lib().hmm_seqshard_mid_reduce(A.data_ptr(), E.data_ptr(), *dims, eps, int(bool(seq_start)), int(R),
                                                    op.data_ptr(), ex.data_ptr(), ws.data_ptr(), ws.numel(),
                                                    engine._stream(E.device)))
    return op, ex


def posterior(A, pi, E_slab, all_ops, all_exps, r, mode=engine.POST_PROB, eps=engine.EPS):
    """Step 3: all_ops (k,b,R,QT,QT) / all_exps (k,b,R,QT) = every rank's slab operators in time order
    -> (out (k,b,Ls,q) per `mode`, loglik (k,b) fp64 of the WHOLE sequences, the same bits on every rank, phi (k,b)
    fp32: this slab's share of the floor-transition bound, +inf for a model whose support is not primitive)."""
    A, pi, E = engine._dev(A, "A"), engine._dev(pi, "pi"), engine._dev(E_slab, "E_slab")
    all_ops = engine._dev(all_ops, "all_ops", align=16)
    all_exps = engine._dev(all_exps, "all_exps", torch.int32)
    A, pi, dims = _shapes(A, E, pi)
    k, b, _, q = dims
    R = all_ops.shape[2] if all_ops.dim() == 5 else 0
    with torch.cuda.device(E.device):
        ws = _ws(dims, R, E.device)
        QT = tile(q)
        if tuple(all_ops.shape) != (k, b, R, QT, QT) or tuple(all_exps.shape) != (k, b, R, QT):
            raise ValueError("all_ops / all_exps must have shapes (k,b,R,%d,%d) / (k,b,R,%d)" % (QT, QT, QT))
        out = torch.empty_like(E)
        ll = torch.empty((k, b), dtype=torch.float64, device=E.device)
        phi = torch.empty((k, b), dtype=torch.float32, device=E.device)
        engine._check(lib().hmm_seqshard_mid_posterior(A.data_ptr(), pi.data_ptr(), E.data_ptr(), *dims, eps, int(r == 0),
                                                       all_ops.data_ptr(), all_exps.data_ptr(), int(R), int(r), int(mode),
                                                       out.data_ptr(), ll.data_ptr(), phi.data_ptr(), ws.data_ptr(),
                                                       ws.numel(), engine._stream(E.device)))
    return out, ll, phi


class MidEngineBackend:
    """The local steps of seqshard.posterior() on the HIP engine for 17 to 64 states (through the C ABI)."""

    def reduce(self, A, E_slab, seq_start, R):
        return reduce(A, E_slab, seq_start, R)

    def posterior(self, A, pi, E_slab, all_ops, all_exps, r, mode):
        return posterior(A, pi, E_slab, all_ops, all_exps, r, mode=mode)

    def unsharded(self, A, pi, E, mode):
        return engine.posterior(A, pi, E, mode=mode)
