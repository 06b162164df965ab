"""Sequence-sharded Viterbi for up to 64 states: the ctypes binding of hmm_seqshard_vscan_* (include/hmm_engine.h).

The protocol is seqshard.viterbi's (reduce, all-gather, apply, all-gather, path) with hmm_viterbi_scan's q x q max-plus
operators in tiles of QT = tile(q) = 32 or 64 states; seqshard.viterbi picks this backend for 17 to 64 states.  The
symbols are typed here, on the handle engine.lib() returns, and keep a signature table of their own (SIGNATURES);
everything else — device checks, the workspace cache, the stream, error codes — is engine's.  No CPU compute.
"""
import torch

from . import engine
from .engine import _I, _P, _SZ

# symbol -> (restype, argtypes)
SIGNATURES = {
    "hmm_seqshard_vscan_max_states": (_I, []),
    "hmm_seqshard_vscan_tile": (_I, [_I]),
    "hmm_seqshard_vscan_workspace_bytes": (_SZ, [_I] * 5),
    "hmm_seqshard_vscan_reduce": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _P, _P, _SZ, _P]),
    "hmm_seqshard_vscan_apply": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _P, _P, _I, _I, _P, _P, _P, _P, _SZ, _P]),
    "hmm_seqshard_vscan_path": (_I, [_I, _I, _I, _I, _P, _P, _I, _I, _P, _P, _SZ, _P]),
}
WORKSPACE_TAG = "seqshard_vscan"
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
    return lib().hmm_seqshard_vscan_max_states()


def tile(q):
    """Edge of the exchanged operators: 32 for q <= 32, 64 up to 64 states; 0 outside 1 .. 64."""
    return lib().hmm_seqshard_vscan_tile(int(q))


def _ws(dims, R, device):
    q = dims[3]
    if q > max_states():
        raise ValueError("sequence-sharded Viterbi covers q <= %d states, got %d" % (max_states(), q))
    need = lib().hmm_seqshard_vscan_workspace_bytes(*dims, int(R))
    if need == 0:
        raise ValueError("bad sequence-sharded Viterbi call: (k, b, Ls, q) = %s, R = %d" % (tuple(dims), R))
    return engine._workspace(device, need, WORKSPACE_TAG)


def reduce(logA, logpi, logE_slab, seq_start, R):
    """Step 1: this rank's time slab logE_slab (k,b,Ls,q) of log-probabilities -> its max-plus operator per sequence,
    slab_vop (k,b,QT,QT) int32 (every column below q has maximum 0) and slab_vbase (k,b,QT) int64.  The chunk operators
    stay in this device's "seqshard_vscan" workspace (one per stream) for apply()."""
    logA, logpi, logE, dims = engine._log_model(logA, logpi, logE_slab)
    k, b, _, q = dims
    with torch.cuda.device(logE.device):
        ws = _ws(dims, R, logE.device)
        QT = tile(q)
        vop = torch.empty((k, b, QT, QT), dtype=torch.int32, device=logE.device)
        vbase = torch.empty((k, b, QT), dtype=torch.int64, device=logE.device)
        engine._check(lib().hmm_seqshard_vscan_reduce(logA.data_ptr(), logpi.data_ptr(), logE.data_ptr(), *dims,
                                                      int(bool(seq_start)), int(R), vop.data_ptr(), vbase.data_ptr(),
                                                      ws.data_ptr(), ws.numel(), engine._stream(logE.device)))
    return vop, vbase


def apply(logA, logpi, logE_slab, all_vops, all_vbases, r):
    """Step 3: all_vops (k,b,R,QT,QT) int32 / all_vbases (k,b,R,QT) int64 = every rank's slab operators in time order
    -> (origin (k,b,QT) uint8: the state before the slab of the best path into every state at the slab's last
    position; final_state (k,b) int32 and score (k,b) fp64 of the WHOLE sequences, the same on every rank).  The
    backpointers stay in the workspace for path()."""
    logA, logpi, logE, dims = engine._log_model(logA, logpi, logE_slab)
    all_vops = engine._dev(all_vops, "all_vops", torch.int32, align=16)
    all_vbases = engine._dev(all_vbases, "all_vbases", torch.int64)
    k, b, _, q = dims
    R = all_vops.shape[2] if all_vops.dim() == 5 else 0
    with torch.cuda.device(logE.device):
        ws = _ws(dims, R, logE.device)
        QT = tile(q)
        if tuple(all_vops.shape) != (k, b, R, QT, QT) or tuple(all_vbases.shape) != (k, b, R, QT):
            raise ValueError("all_vops / all_vbases must have shapes (k,b,R,%d,%d) / (k,b,R,%d)" % (QT, QT, QT))
        origin = torch.empty((k, b, QT), dtype=torch.uint8, device=logE.device)
        final_state = torch.empty((k, b), dtype=torch.int32, device=logE.device)
        score = torch.empty((k, b), dtype=torch.float64, device=logE.device)
        engine._check(lib().hmm_seqshard_vscan_apply(logA.data_ptr(), logpi.data_ptr(), logE.data_ptr(), *dims, int(r == 0),
                                                     all_vops.data_ptr(), all_vbases.data_ptr(), int(R), int(r),
                                                     origin.data_ptr(), final_state.data_ptr(), score.data_ptr(),
                                                     ws.data_ptr(), ws.numel(), engine._stream(logE.device)))
    return origin, final_state, score


def path(dims, all_origins, final_state, r):
    """Step 5: dims = (k, b, Ls, q) of this rank's slab, all_origins (k,b,R,QT) uint8 = every rank's origin in time
    order, final_state (k,b) int32 -> path (k,b,Ls) int32, this slab's piece of the most probable path."""
    k, b, Ls, q = (int(d) for d in dims)
    all_origins = engine._dev(all_origins, "all_origins", torch.uint8)
    final_state = engine._dev(final_state, "final_state", torch.int32)
    R = all_origins.shape[2] if all_origins.dim() == 4 else 0
    device = all_origins.device
    with torch.cuda.device(device):
        ws = _ws((k, b, Ls, q), R, device)
        QT = tile(q)
        if tuple(all_origins.shape) != (k, b, R, QT) or tuple(final_state.shape) != (k, b):
            raise ValueError("all_origins / final_state must have shapes (k,b,R,%d) / (k,b)" % QT)
        out = torch.empty((k, b, Ls), dtype=torch.int32, device=device)
        engine._check(lib().hmm_seqshard_vscan_path(k, b, Ls, q, all_origins.data_ptr(), final_state.data_ptr(), int(R),
                                                    int(r), out.data_ptr(), ws.data_ptr(), ws.numel(),
                                                    engine._stream(device)))
    return out


class VscanEngineBackend:
    """The local steps of seqshard.viterbi() on the HIP engine for up to 64 states (through the C ABI)."""

    def reduce(self, logA, logpi, logE_slab, seq_start, R):
        return reduce(logA, logpi, logE_slab, seq_start, R)

    def apply(self, logA, logpi, logE_slab, all_vops, all_vbases, r):
        return apply(logA, logpi, logE_slab, all_vops, all_vbases, r)

    def path(self, dims, all_origins, final_state, r):
        return path(dims, all_origins, final_state, r)
