"""ctypes binding of the HIP engine's C ABI (include/hmm_engine.h).

PyTorch is used only for device memory and the current HIP stream.  There is no CPU
fallback: if the library is missing or a tensor is not on a HIP device these functions
raise.  Shapes follow the reference (k models, b sequences, L positions, q states):
A (k,q,q), pi (k,q) or (1,k,q), E (k,b,L,q).
"""
import contextlib
import ctypes
import os

import torch

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG, "libhmm_engine.so")

OP_LOGLIK, OP_FORWARD, OP_BACKWARD, OP_POSTERIOR, OP_VITERBI = 0, 1, 2, 3, 4
POST_PROB, POST_LOG, POST_LOG_NO_LL = 0, 1, 2
EPS = 1e-16
ABI_VERSION = 3
# tuning / test options (include/hmm_engine.h: HMM_OPT_*, HMM_EXACT_*)
OPT_CHUNK, OPT_FORCE_DENSE, OPT_SCAN2, OPT_GROUPS, OPT_EXACT, OPT_PGCHUNK, OPT_VGROUPS = 0, 1, 2, 3, 4, 5, 6
OPT_VLARGE = 7          # viterbi_large: 0 = by q, 1 = per-sequence walk, 2 = per-position tiles
OPT_GLARGE = 8          # loglik_grad_large, posterior_grad_large: 0 = by q, 1 = per-sequence walk, 2 = per-position GEMMs
EXACT_AUTO, EXACT_OFF, EXACT_ALWAYS, EXACT_ALWAYS_NARROW = 0, 1, 2, 3

_lib = None
_workspaces = {}


class EngineError(RuntimeError):
    pass


_P, _I, _F, _SZ, _LL = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t, ctypes.c_longlong
_FORWARD = [_P, _P, _P, _I, _I, _I, _I, _F, _P, _P, _P, _SZ, _P]
_POSTERIOR = [_P, _P, _P, _I, _I, _I, _I, _F, _I, _P, _P, _P, _SZ, _P]
_VITERBI = [_P, _P, _P, _I, _I, _I, _I, _P, _P, _P, _SZ, _P]
_LOGLIK_GRAD = [_P, _P, _P, _I, _I, _I, _I, _F, _P, _P, _P, _P, _P, _P, _SZ, _P]
_POSTERIOR_GRAD = [_P, _P, _P, _I, _I, _I, _I, _F, _I, _P, _P, _P, _P, _P, _SZ, _P]
_EMITTER = [_P, _I, _I, _I, _P, _I, _P, _P, _I, _P, _I, _F, _F, _I]
_LAST_CALL = [_I, _I, _I, _I, _P, _SZ]          # (k, b, L, q, workspace, bytes): readers of the last call's records

# Every function of include/hmm_engine.h that this module calls: symbol -> (restype, argtypes).
_SIGNATURES = {
    "hmm_strerror": (ctypes.c_char_p, [_I]),
    "hmm_abi_version": (_I, []),
    "hmm_set_option": (_I, [_I, _I]),
    "hmm_get_option": (_I, [_I]),
    "hmm_max_states": (_I, []),
    "hmm_scan_max_states": (_I, []),
    "hmm_largeq_tile_cols": (_I, [_I, _I]),
    "hmm_chunk_len": (_I, [_I] * 4),
    "hmm_plan_capacity": (_I, [_I]),
    "hmm_plan_capacity_device": (_I, [_I]),
    "hmm_workspace_bytes": (_SZ, [_I] * 5),
    "hmm_forward": (_I, _FORWARD),
    "hmm_backward": (_I, [_P, _P, _I, _I, _I, _I, _F, _P, _P, _SZ, _P]),
    "hmm_posterior": (_I, _POSTERIOR),
    "hmm_exact_count": (_LL, [_I] + _LAST_CALL),
    "hmm_exact_detail_op": (_I, [_I] + _LAST_CALL + [_P]),
    "hmm_window_table": (_I, [_I] + _LAST_CALL + [_I, _P, _P, _P, _I]),
    "hmm_profile_create": (_P, []),
    "hmm_profile_destroy": (None, [_P]),
    "hmm_posterior_profiled": (_I, _POSTERIOR + [_P]),
    "hmm_profile_read": (_I, [_P, _P, _P]),
    "hmm_viterbi_max_states": (_I, []),
    "hmm_viterbi_workspace_bytes": (_SZ, [_I] * 4),
    "hmm_viterbi": (_I, _VITERBI),
    "hmm_viterbi_scan_max_states": (_I, []),
    "hmm_viterbi_scan_chunk_len": (_I, [_I] * 4),
    "hmm_viterbi_scan_pays": (_I, [_I] * 4),
    "hmm_viterbi_scan_workspace_bytes": (_SZ, [_I] * 4),
    "hmm_viterbi_scan": (_I, _VITERBI),
    "hmm_viterbi_large_max_states": (_I, []),
    "hmm_viterbi_large_workspace_bytes": (_SZ, [_I] * 4),
    "hmm_viterbi_large": (_I, _VITERBI),
    "hmm_grad_max_states": (_I, []),
    "hmm_loglik_grad_workspace_bytes": (_SZ, [_I] * 4),
    "hmm_loglik_grad": (_I, _LOGLIK_GRAD),
    "hmm_loglik_grad_serial_count": (_LL, _LAST_CALL),
    "hmm_loglik_grad_scan_max_states": (_I, []),
    "hmm_loglik_grad_scan_chunk_len": (_I, [_I] * 4),
    "hmm_loglik_grad_scan_pays": (_I, [_I] * 4),
    "hmm_loglik_grad_scan_workspace_bytes": (_SZ, [_I] * 4),
    "hmm_loglik_grad_scan_serial_count": (_LL, _LAST_CALL),
    "hmm_loglik_grad_scan": (_I, _LOGLIK_GRAD),
    "hmm_loglik_grad_large_max_states": (_I, []),
    "hmm_loglik_grad_large_workspace_bytes": (_SZ, [_I] * 4),
    "hmm_loglik_grad_large": (_I, _LOGLIK_GRAD),
    "hmm_posterior_grad_max_states": (_I, []),
    "hmm_posterior_grad_workspace_bytes": (_SZ, [_I] * 4),
    "hmm_posterior_grad": (_I, _POSTERIOR_GRAD),
    "hmm_posterior_grad_serial_count": (_LL, _LAST_CALL),
    "hmm_posterior_grad_scan_max_states": (_I, []),
    "hmm_posterior_grad_scan_chunk_len": (_I, [_I] * 4),
    "hmm_posterior_grad_scan_pays": (_I, [_I] * 4),
    "hmm_posterior_grad_scan_workspace_bytes": (_SZ, [_I] * 4),
    "hmm_posterior_grad_scan_serial_count": (_LL, _LAST_CALL),
    "hmm_posterior_grad_scan": (_I, _POSTERIOR_GRAD),
    "hmm_posterior_grad_large_max_states": (_I, []),
    "hmm_posterior_grad_large_workspace_bytes": (_SZ, [_I] * 4),
    "hmm_posterior_grad_large": (_I, _POSTERIOR_GRAD),
    "hmm_gene_emissions": (_I, _EMITTER + [_P, _P]),
    "hmm_gene_emissions_grad_workspace_bytes": (_SZ, [_I] * 5),
    "hmm_gene_emissions_grad": (_I, _EMITTER + [_P, _P, _P, _P, _SZ, _P]),
    "hmm_gene_emissions_wide_max_states": (_I, []),
    "hmm_gene_emissions_wide": (_I, _EMITTER + [_P, _P]),
    "hmm_gene_emissions_grad_wide_workspace_bytes": (_SZ, [_I] * 5),
    "hmm_gene_emissions_grad_wide": (_I, _EMITTER + [_P, _P, _P, _P, _SZ, _P]),
    "hmm_embedding_emissions_max_dim": (_I, []),
    "hmm_embedding_emissions": (_I, [_P, _LL, _I, _I, _I, _P, _P, _P, _I, _P, _I, _F, _F, _I, _P, _P]),
    "hmm_embedding_emissions_grad_max_dim": (_I, []),
    "hmm_embedding_emissions_grad_workspace_bytes": (_SZ, [_I] * 5),
    "hmm_embedding_emissions_grad": (_I, [_P, _LL, _I, _I, _I, _P, _P, _P, _I, _P, _I, _F, _F, _P, _P, _P, _P, _LL,
                                          _P, _P, _P, _P, _SZ, _P]),
    "hmm_embedding_emissions_wide_max_states": (_I, []),
    "hmm_embedding_emissions_wide": (_I, [_P, _LL, _I, _I, _I, _P, _P, _P, _I, _P, _I, _F, _F, _I, _P, _P]),
    "hmm_embedding_emissions_grad_wide_workspace_bytes": (_SZ, [_I] * 5),
    "hmm_embedding_emissions_grad_wide": (_I, [_P, _LL, _I, _I, _I, _P, _P, _P, _I, _P, _I, _F, _F, _P, _P, _P, _P, _LL,
                                               _P, _P, _P, _P, _SZ, _P]),
    "hmm_nucleotide_emissions_max_states": (_I, []),
    "hmm_nucleotide_emissions": (_I, [_P, _LL, _I, _I, _P, _I, _P, _I, _F, _I, _P, _P]),
    "hmm_nucleotide_emissions_grad_workspace_bytes": (_SZ, [_I] * 4),
    "hmm_nucleotide_emissions_grad": (_I, [_P, _LL, _I, _I, _P, _I, _P, _I, _F, _P, _P, _P, _P, _P, _SZ, _P]),
    "hmm_loglik_partials": (_I, [_P, _P, _I, _I, _P, _P]),
    "hmm_loglik_allreduce": (_I, [_P, _P, _I, _P]),
    "hmm_seqshard_workspace_bytes": (_SZ, [_I] * 5),
    "hmm_seqshard_reduce": (_I, [_P, _P, _I, _I, _I, _I, _F, _I, _I, _P, _P, _P, _SZ, _P]),
    "hmm_seqshard_posterior": (_I, [_P, _P, _P, _I, _I, _I, _I, _F, _I, _P, _P, _I, _I, _I, _P, _P, _P, _P, _SZ, _P]),
    "hmm_seqshard_viterbi_max_states": (_I, []),
    "hmm_seqshard_viterbi_workspace_bytes": (_SZ, [_I] * 5),
    "hmm_seqshard_viterbi_reduce": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _P, _P, _SZ, _P]),
    "hmm_seqshard_viterbi_apply": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _P, _P, _I, _I, _P, _P, _P, _P, _SZ, _P]),
    "hmm_seqshard_viterbi_path": (_I, [_I, _I, _I, _I, _P, _P, _I, _I, _P, _P, _SZ, _P]),
}

# posterior_decode's symbols, typed by lib() like the table above.  They are kept apart from it as the sequence-sharded
# modules keep theirs: the guard-band table of the test suite is checked against _SIGNATURES, and this entry point's
# guard-band rows and completeness check live in a test file of their own.
DECODE_SIGNATURES = {
    "hmm_posterior_decode_max_states": (_I, []),
    "hmm_posterior_decode": (_I, [_P, _P, _P, _I, _I, _I, _I, _F, _P, _I, _P, _P, _P, _P, _SZ, _P]),
}

# ... and those of the fused decode for 17..64 states (hmm_posterior_decode_mid), apart from both tables above for the
# same reason: each table's guard-band completeness check lives in the test file that has its rows.
DECODE_MID_SIGNATURES = {
    "hmm_posterior_decode_mid_max_states": (_I, []),
    "hmm_posterior_decode_mid_workspace_bytes": (_SZ, [_I, _I, _I, _I]),
    "hmm_posterior_decode_mid": (_I, [_P, _P, _P, _I, _I, _I, _I, _F, _P, _I, _P, _P, _P, _P, _SZ, _P]),
}

# ... and those of the per-sequence walk for 65..256 states (hmm_posterior_walk, hmm_posterior_decode_wide), in a table
# of their own for the same reason.
POSTERIOR_WALK_SIGNATURES = {
    "hmm_posterior_walk_min_states": (_I, []),
    "hmm_posterior_walk_max_states": (_I, []),
    "hmm_posterior_walk_workspace_bytes": (_SZ, [_I, _I, _I, _I]),
    "hmm_posterior_walk_pays": (_I, [_I, _I, _I, _I]),
    "hmm_posterior_walk": (_I, _POSTERIOR),
    "hmm_posterior_decode_wide_workspace_bytes": (_SZ, [_I, _I, _I, _I]),
    "hmm_posterior_decode_wide": (_I, [_P, _P, _P, _I, _I, _I, _I, _F, _P, _I, _P, _P, _P, _P, _SZ, _P]),
}

# ... and those of the training walk for 65..256 states (hmm_loglik_grad_walk), in a table of their own for the same
# reason.
LOGLIK_GRAD_WALK_SIGNATURES = {
    "hmm_loglik_grad_walk_min_states": (_I, []),
    "hmm_loglik_grad_walk_max_states": (_I, []),
    "hmm_loglik_grad_walk_workspace_bytes": (_SZ, [_I, _I, _I, _I]),
    "hmm_loglik_grad_walk_pays": (_I, [_I, _I, _I, _I]),
    "hmm_loglik_grad_walk_refused": (_LL, _LAST_CALL),
    "hmm_loglik_grad_walk": (_I, _LOGLIK_GRAD),
}

# ... and those of the posterior-gradient walk for 65..256 states (hmm_posterior_grad_walk), likewise.
POSTERIOR_GRAD_WALK_SIGNATURES = {
    "hmm_posterior_grad_walk_min_states": (_I, []),
    "hmm_posterior_grad_walk_max_states": (_I, []),
    "hmm_posterior_grad_walk_workspace_bytes": (_SZ, [_I, _I, _I, _I]),
    "hmm_posterior_grad_walk_pays": (_I, [_I, _I, _I, _I]),
    "hmm_posterior_grad_walk_refused": (_LL, _LAST_CALL),
    "hmm_posterior_grad_walk": (_I, _POSTERIOR_GRAD),
}

# ... and those of the class posteriors with gradients for 65..256 states (hmm_class_posterior_walk,
# hmm_class_posterior_grad_walk), likewise.
CLASS_POSTERIOR_WALK_SIGNATURES = {
    "hmm_class_posterior_walk_workspace_bytes": (_SZ, [_I, _I, _I, _I]),
    "hmm_class_posterior_walk_pays": (_I, [_I, _I, _I, _I]),
    "hmm_class_posterior_walk": (_I, [_P, _P, _P, _I, _I, _I, _I, _F, _P, _I, _P, _P, _P, _P, _SZ, _P]),
    "hmm_class_posterior_grad_walk_workspace_bytes": (_SZ, [_I, _I, _I, _I, _I]),
    "hmm_class_posterior_grad_walk": (_I, [_P, _P, _P, _I, _I, _I, _I, _F, _I, _P, _I, _P, _P, _P, _P, _P, _P, _SZ, _P]),
}

# ... and those of the class posteriors with gradients for up to 16 states (hmm_class_posterior,
# hmm_class_posterior_grad), likewise.
CLASS_POSTERIOR_SIGNATURES = {
    "hmm_class_posterior_max_states": (_I, []),
    "hmm_class_posterior_workspace_bytes": (_SZ, [_I, _I, _I, _I]),
    "hmm_class_posterior_pays": (_I, [_I, _I, _I, _I]),
    "hmm_class_posterior": (_I, [_P, _P, _P, _I, _I, _I, _I, _F, _P, _I, _P, _P, _P, _P, _SZ, _P]),
    "hmm_class_posterior_grad_workspace_bytes": (_SZ, [_I, _I, _I, _I, _I]),
    "hmm_class_posterior_grad_pays": (_I, [_I, _I, _I, _I]),
    "hmm_class_posterior_grad": (_I, [_P, _P, _P, _I, _I, _I, _I, _F, _I, _P, _I, _P, _P, _P, _P, _P, _P, _SZ, _P]),
}


def lib():
    """The loaded shared library (loaded once).  Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise EngineError(
            "HIP engine library %s is missing: build it with `python -m hmm_layer_amd.build` "
            "(there is no CPU fallback)" % LIB_PATH)
    L = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in {**_SIGNATURES, **DECODE_SIGNATURES, **DECODE_MID_SIGNATURES,
                                      **POSTERIOR_WALK_SIGNATURES, **LOGLIK_GRAD_WALK_SIGNATURES,
                                      **POSTERIOR_GRAD_WALK_SIGNATURES, **CLASS_POSTERIOR_WALK_SIGNATURES,
                                      **CLASS_POSTERIOR_SIGNATURES}.items():
        if not hasattr(L, name):
            raise EngineError("the engine library %s does not export %s: rebuild it with "
                              "`python -m hmm_layer_amd.build`" % (LIB_PATH, name))
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = L
    return L


def _check(rc):
    if rc != 0:
        raise EngineError("hmm_engine: %s (code %d)" % (lib().hmm_strerror(rc).decode(), rc))


def _dev(t, name, dtype=torch.float32, align=0):
    """The tensor as the C ABI takes it: on a HIP device, of `dtype`, contiguous.  align: for the few arguments whose
    kernels need more than element alignment (include/hmm_engine.h, "Memory contract"), a view that starts elsewhere
    is copied to a fresh tensor."""
    if not torch.is_tensor(t):
        raise TypeError("%s must be a torch.Tensor" % name)
    if not t.is_cuda:
        raise EngineError("%s must live on a HIP device (got %s); the engine has no CPU path" % (name, t.device))
    if t.dtype != dtype:
        raise TypeError("%s must be %s, got %s" % (name, dtype, t.dtype))
    t = t.contiguous()
    return t.clone() if align and t.data_ptr() % align else t


def _shapes(A, E, pi=None):
    if E.dim() != 4:
        raise ValueError("E must have shape (k, b, L, q), got %s" % (tuple(E.shape),))
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
        raise ValueError("empty input: (k, b, L, q) = %s" % ((k, b, L, q),))
    if q > lib().hmm_max_states():
        raise ValueError("q = %d states exceeds the scan kernels' limit of %d" % (q, lib().hmm_max_states()))
    return A, pi, (k, b, L, q)


def _workspace(device, need, tag=None, floor=1 << 20):
    """The cached workspace of (device, current stream[, tag]), grown to at least `need` bytes.  The recursions'
    workspace has no tag; calls that must not overwrite its routing records (exact_count and its kin read
    them) keep theirs under a tag of their own."""
    key = (device.index, torch.cuda.current_stream(device).cuda_stream) + ((tag,) if tag else ())
    ws = _workspaces.get(key)
    if ws is None or ws.numel() < need:
        ws = torch.empty(max(need, floor), dtype=torch.uint8, device=device)
        _workspaces[key] = ws
    return ws


@contextlib.contextmanager
def _last_workspace(device, tag=None):
    """For the readers of the last call's records: on `device` (default: the current one), the recursions'
    workspace of the current stream (or the one kept under `tag`), with the stream synchronised."""
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else device
    with torch.cuda.device(device):
        ws = _workspaces.get((device.index, torch.cuda.current_stream(device).cuda_stream) + ((tag,) if tag else ()))
        if ws is None:
            raise EngineError("no call has run on this device / stream yet")
        torch.cuda.current_stream(device).synchronize()
        yield ws


def release_workspaces():
    _workspaces.clear()


def _stream(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def chunk_len(k, b, L, q):
    return lib().hmm_chunk_len(k, b, L, q)


def plan_capacity():
    """What the chunk rule takes the machine to hold (constants of the build) ->
    dict(cus, forward_blocks_per_cu, backward_blocks_per_cu, reduce_blocks_per_cu).  No device needed."""
    return _plan_capacity(lib().hmm_plan_capacity)


def plan_capacity_device(device=None):
    """The same read from the device: its compute units and the occupancy query's blocks per compute unit."""
    with torch.cuda.device(device if device is not None else torch.cuda.current_device()):
        return _plan_capacity(lib().hmm_plan_capacity_device)


def _plan_capacity(fn):
    out = {}
    for which, name in enumerate(("cus", "forward_blocks_per_cu", "backward_blocks_per_cu", "reduce_blocks_per_cu")):
        out[name] = int(fn(which))
        if out[name] < 0:
            _check(out[name])
    return out


def largeq_tile_cols(b, q):
    """Column width of the GEMM tile serving (b sequences per model, q > 64 states); 0 otherwise."""
    return lib().hmm_largeq_tile_cols(int(b), int(q))


def set_option(option, value):
    """Sets a process-wide tuning / test option (OPT_*); returns the previous value."""
    if not 0 <= int(option) <= OPT_GLARGE:
        raise ValueError("unknown option %r" % (option,))
    return lib().hmm_set_option(int(option), int(value))


def get_option(option):
    return lib().hmm_get_option(int(option))


class option:
    """Context manager: `with engine.option(engine.OPT_CHUNK, 64): ...` (tests and A/B scripts)."""

    def __init__(self, opt, value):
        self.opt, self.value = opt, value

    def __enter__(self):
        self.old = set_option(self.opt, self.value)
        return self

    def __exit__(self, *exc):
        set_option(self.opt, self.old)
        return False


def exact_count(op, dims, device=None, tag=None):
    """How many of the k*b sequences of the LAST q <= 16 call of kind `op` with shape `dims` on this
    device and stream were served by the serial exact-clamp kernels (synchronises).  tag=DECODE_TAG (with
    OP_POSTERIOR) reads the last posterior_decode() call instead of the last posterior()."""
    with _last_workspace(device, tag) as ws:
        n = lib().hmm_exact_count(int(op), *dims, ws.data_ptr(), ws.numel())
    if n < 0:
        _check(int(n))
    return int(n)


def exact_detail(dims, device=None, op=OP_POSTERIOR, tag=None):
    """Routing of the LAST posterior() call (q <= 16) with shape `dims` on this device and stream ->
    dict(routed=sequences that left the scan, window_sequences=..., windows=..., whole=sequences redone whole,
    window_chunks=chunks the windows walked).  Synchronises.  op: OP_LOGLIK / OP_FORWARD (forward() without / with
    log alpha) or OP_BACKWARD for the last call of those entry points instead; tag=DECODE_TAG for the last
    posterior_decode() call."""
    with _last_workspace(device, tag) as ws:
        d = (ctypes.c_longlong * 5)()
        _check(lib().hmm_exact_detail_op(int(op), *[int(x) for x in dims], ws.data_ptr(), ws.numel(), d))
    return dict(routed=int(d[0]), window_sequences=int(d[1]), windows=int(d[2]), whole=int(d[3]), window_chunks=int(d[4]))


def window_table(dims, seq, op=OP_POSTERIOR, device=None, tag=None):
    """Diagnostics (q <= 16): the windows of sequence `seq` (index into k*b) after the LAST call of `op` with shape `dims`
    on this device and stream -> dict(windows=[(first chunk, chunks), ...], shifts=[log-scale shift per window]
    (OP_FORWARD / OP_BACKWARD), psi=numpy array of the per-chunk certificate sums; chunks the reduce marked for having
    gone through the denormal range read 1.0).  Synchronises.  tag=DECODE_TAG: the last posterior_decode() call."""
    import numpy as np
    with _last_workspace(device, tag) as ws:
        k, b, L, q = (int(x) for x in dims)
        C = (L + chunk_len(k, b, L, q) - 1) // chunk_len(k, b, L, q)
        tab = (ctypes.c_int * 34)()
        sh = (ctypes.c_double * 24)()
        ps = (ctypes.c_float * C)()
        rc = lib().hmm_window_table(int(op), k, b, L, q, ws.data_ptr(), ws.numel(), int(seq), tab, sh, ps, C)
        if rc < 0:
            _check(rc)
    n = max(0, min(int(tab[0]), 16))
    return dict(windows=[(int(tab[2 + 2 * i]), int(tab[3 + 2 * i]) & 0xFFFFFF) for i in range(n)],
                shifts=[float(sh[i]) for i in range(n)], psi=np.array(ps[:], dtype=np.float32))


def loglik_grad_serial_count(dims, device=None):
    """The same for the LAST loglik_grad call (17..64 states) that hmm_loglik_grad itself served."""
    return posterior_grad_serial_count(dims, device, _fn="hmm_loglik_grad_serial_count")


def loglik_grad_scan_serial_count(dims, device=None):
    """The same for the LAST loglik_grad_scan call (also one that loglik_grad routed there)."""
    return posterior_grad_serial_count(dims, device, _fn="hmm_loglik_grad_scan_serial_count", _tag="loglik_grad_scan")


def posterior_grad_scan_serial_count(dims, device=None):
    """The same for the LAST posterior_grad_scan call (also one that posterior_grad routed there)."""
    return posterior_grad_serial_count(dims, device, _fn="hmm_posterior_grad_scan_serial_count", _tag="posterior_grad_scan")


def posterior_grad_serial_count(dims, device=None, _fn="hmm_posterior_grad_serial_count", _tag=None):
    """How many of the k*b sequences of the LAST posterior_grad call with shape `dims` on this device and
    stream were served by the whole-sequence sweeps rather than per chunk (synchronises)."""
    with _last_workspace(device, _tag) as ws:
        n = getattr(lib(), _fn)(*[int(d) for d in dims], ws.data_ptr(), ws.numel())
    if n < 0:
        _check(int(n))
    return int(n)


def forward(A, pi, E, want_log_alpha=True, eps=EPS):
    """-> (log_alpha (k,b,L,q) fp32 or None, loglik (k,b) fp64)."""
    A, pi, E = _dev(A, "A"), _dev(pi, "pi"), _dev(E, "E")
    A, pi, dims = _shapes(A, E, pi)
    with torch.cuda.device(E.device):
        ws = _workspace(E.device, lib().hmm_workspace_bytes(OP_FORWARD if want_log_alpha else OP_LOGLIK, *dims))
        la = torch.empty_like(E) if want_log_alpha else None
        ll = torch.empty(dims[:2], dtype=torch.float64, device=E.device)
        _check(lib().hmm_forward(A.data_ptr(), pi.data_ptr(), E.data_ptr(), *dims, eps,
                                 la.data_ptr() if want_log_alpha else None, ll.data_ptr(),
                                 ws.data_ptr(), ws.numel(), _stream(E.device)))
    return la, ll


def backward(A, E, eps=EPS):
    """-> log_beta (k,b,L,q) fp32."""
    A, E = _dev(A, "A"), _dev(E, "E")
    A, _, dims = _shapes(A, E)
    with torch.cuda.device(E.device):
        ws = _workspace(E.device, lib().hmm_workspace_bytes(OP_BACKWARD, *dims))
        lb = torch.empty_like(E)
        _check(lib().hmm_backward(A.data_ptr(), E.data_ptr(), *dims, eps, lb.data_ptr(),
                                  ws.data_ptr(), ws.numel(), _stream(E.device)))
    return lb


KERNELS = ("reduce", "scan", "forward", "backward", "exact")


class Profile:
    """Per-kernel HIP-event timing of posterior() calls (bench.py's roofline leg)."""

    def __init__(self):
        self.handle = ctypes.c_void_p(lib().hmm_profile_create())

    def read(self):
        """-> {kernel: (total ms, launches)} since the last read; waits for the events."""
        ms = (ctypes.c_double * len(KERNELS))()
        n = (ctypes.c_longlong * len(KERNELS))()
        _check(lib().hmm_profile_read(self.handle, ms, n))
        return {name: (ms[i], n[i]) for i, name in enumerate(KERNELS)}

    def close(self):
        if self.handle:
            lib().hmm_profile_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def posterior(A, pi, E, mode=POST_PROB, eps=EPS, out=None, profile=None):
    """-> (posterior (k,b,L,q) fp32 per `mode`, loglik (k,b) fp64)."""
    A, pi, E = _dev(A, "A"), _dev(pi, "pi"), _dev(E, "E")
    A, pi, dims = _shapes(A, E, pi)
    with torch.cuda.device(E.device):
        ws = _workspace(E.device, lib().hmm_workspace_bytes(OP_POSTERIOR, *dims))
        if out is None:
            out = torch.empty_like(E)
        elif (out.shape != E.shape or out.dtype != torch.float32 or not out.is_contiguous()
              or out.device != E.device):
            raise ValueError("out must be a contiguous fp32 tensor shaped like E on E's device")
        ll = torch.empty(dims[:2], dtype=torch.float64, device=E.device)
        args = (A.data_ptr(), pi.data_ptr(), E.data_ptr(), *dims, eps, int(mode),
                out.data_ptr(), ll.data_ptr(), ws.data_ptr(), ws.numel(), _stream(E.device))
        if profile is None:
            _check(lib().hmm_posterior(*args))
        else:
            _check(lib().hmm_posterior_profiled(*args, profile.handle))
    return out, ll


def posterior_walk(A, pi, E, mode=POST_LOG, eps=EPS):
    """-> (posterior (k,b,L,q) fp32 per `mode`, loglik (k,b) fp64) by the per-sequence walk for 65..256 states
    (hmm_posterior_walk): one workgroup per sequence with the cell's exact step, the sparse step for models whose
    states have at most 8 predecessors and successors apart from two hubs.  posterior() keeps its per-position GEMMs
    in this range; the two agree to rounding order.  Raises ValueError outside 65..256 states."""
    lo, hi = lib().hmm_posterior_walk_min_states(), lib().hmm_posterior_walk_max_states()
    if torch.is_tensor(E) and E.dim() == 4 and not lo <= E.shape[3] <= hi:     # (before the device is asked for)
        raise ValueError("posterior_walk serves %d..%d states, got q = %d" % (lo, hi, E.shape[3]))
    if int(mode) not in (POST_PROB, POST_LOG, POST_LOG_NO_LL):
        raise ValueError("unknown mode %r" % (mode,))
    A, pi, E = _dev(A, "A"), _dev(pi, "pi"), _dev(E, "E")
    A, pi, dims = _shapes(A, E, pi)
    with torch.cuda.device(E.device):
        ws = _workspace(E.device, lib().hmm_posterior_walk_workspace_bytes(*dims), WALK_TAG)
        out = torch.empty_like(E)
        ll = torch.empty(dims[:2], dtype=torch.float64, device=E.device)
        _check(lib().hmm_posterior_walk(A.data_ptr(), pi.data_ptr(), E.data_ptr(), *dims, eps, int(mode),
                                        out.data_ptr(), ll.data_ptr(), ws.data_ptr(), ws.numel(), _stream(E.device)))
    return out, ll


WALK_TAG = "posterior_walk"          # posterior_walk()'s workspace
DECODE_TAG = "posterior_decode"      # posterior_decode()'s workspace: its routing records survive a posterior() call


def class_table(state_class, num_classes, q):
    """The class map of posterior_decode as (list of q ints or None, number of classes): `state_class` a sequence or
    an integer tensor on any device (brought to the host here, once), None = the identity map."""
    if state_class is None:
        if num_classes is not None and int(num_classes) != q:
            raise ValueError("without state_class every state is its own class: num_classes must be q = %d" % q)
        return None, q
    table = [int(c) for c in (state_class.detach().cpu().reshape(-1).tolist() if torch.is_tensor(state_class)
                              else state_class)]
    if len(table) != q:
        raise ValueError("state_class must have q = %d entries, got %d" % (q, len(table)))
    C = max(table) + 1 if num_classes is None else int(num_classes)
    if C < 1 or min(table) < 0 or max(table) >= C:
        raise ValueError("state_class entries must lie in 0 .. num_classes-1 = %d" % (C - 1))
    return table, C


def collapse_posterior(gamma, table, C):
    """Class sums (..., C) of a posterior tensor (..., q) with torch ops: index_add_ over the state axis by the class
    map `table` (a list of q ints).  Differentiable."""
    idx = torch.tensor(table, dtype=torch.long, device=gamma.device)
    return torch.zeros(gamma.shape[:-1] + (C,), dtype=gamma.dtype, device=gamma.device).index_add_(-1, idx, gamma)


def decode_posterior(gamma, table, C):
    """What posterior_decode computes, from a posterior tensor (..., q) with torch ops: class sums (index_add_ over the
    state axis), then the largest class per position, the lowest index on ties -> (label uint8, conf)."""
    if table is not None:
        gamma = collapse_posterior(gamma, table, C)
    # (torch.argmax returns the first maximal index; torch.max's index is not specified on ties)
    return gamma.argmax(dim=-1).to(torch.uint8), gamma.max(dim=-1).values


def posterior_decode(A, pi, E, state_class=None, num_classes=None, eps=EPS, want_conf=True, sparse=False):
    """Posterior decoding -> (label (k,b,L) uint8, conf (k,b,L) fp32 or None, loglik (k,b) fp64): per position the
    class with the largest posterior (the sum of the state posteriors of its states; the lowest class on ties) and
    that posterior.  Up to 64 states the engine's kernels produce the labels themselves and the (k,b,L,q) tensor is
    never written (hmm_posterior_decode up to 16 states, hmm_posterior_decode_mid for 17..64 with the identity map or
    at most 16 classes; the latter's workspace holds a parking region as large as that tensor, see the header).
    For 65..256 states, with the identity map or at most 16 classes, the per-sequence walk does the same
    (hmm_posterior_decode_wide, same parking region) where hmm_posterior_walk_pays says that it measured faster than
    the composition, for models of up to 128 states and, with `sparse=True`, up to 256: `sparse` is the caller's
    statement that every state of A has at most 8 non-zero predecessors and successors apart from two hubs (the gene
    models), so that the walk takes its sparse step — its dense step above 128 states is slow.
    Everything else — more than 256 states, more than 16 classes above 16 states, a shape where the walk does not
    pay — composes posterior(POST_PROB) with torch ops (same shapes, dtypes and tie rule); the number of classes is
    then limited to 256, the range of a label.  The fused call's workspace is cached per (device, stream) like every
    workspace of this module; above 16 states it is as large as the posterior tensor and stays allocated until
    release_workspaces()."""
    A, pi, E = _dev(A, "A"), _dev(pi, "pi"), _dev(E, "E")
    A, pi, dims = _shapes(A, E, pi)
    q = dims[3]
    table, C = class_table(state_class, num_classes, q)
    small = q <= lib().hmm_posterior_decode_max_states()
    mid = not small and q <= lib().hmm_posterior_decode_mid_max_states()
    wide = (lib().hmm_posterior_walk_min_states() <= q <= lib().hmm_posterior_walk_max_states()
            and (q <= 128 or sparse) and lib().hmm_posterior_walk_pays(*dims) == 1)
    if not small and (not (mid or wide) or (table is not None and C > 16)):
        if C > 256:
            raise ValueError("labels are bytes: at most 256 classes, got %d" % C)
        gamma, ll = posterior(A, pi, E, POST_PROB, eps)
        label, conf = decode_posterior(gamma, table, C)
        return label, (conf if want_conf else None), ll
    if small and C > 16:
        raise ValueError("at most 16 classes, got %d" % C)
    nbytes = (lib().hmm_workspace_bytes(OP_POSTERIOR, *dims) if small
              else lib().hmm_posterior_decode_mid_workspace_bytes(*dims) if mid
              else lib().hmm_posterior_decode_wide_workspace_bytes(*dims))
    call = (lib().hmm_posterior_decode if small else lib().hmm_posterior_decode_mid if mid
            else lib().hmm_posterior_decode_wide)
    with torch.cuda.device(E.device):
        ws = _workspace(E.device, nbytes, DECODE_TAG)
        label = torch.empty(dims[:3], dtype=torch.uint8, device=E.device)
        conf = torch.empty(dims[:3], dtype=torch.float32, device=E.device) if want_conf else None
        ll = torch.empty(dims[:2], dtype=torch.float64, device=E.device)
        tab = (ctypes.c_int * q)(*table) if table is not None else None
        _check(call(A.data_ptr(), pi.data_ptr(), E.data_ptr(), *dims, eps, tab, C,
                    label.data_ptr(), conf.data_ptr() if want_conf else None, ll.data_ptr(),
                    ws.data_ptr(), ws.numel(), _stream(E.device)))
    return label, conf, ll


def _emitter_args(x, B, state_row, codon, state_codon):
    """Validation shared by gene_emissions and gene_emissions_grad -> (the five tensors, (b, L, s, rows, q, nc))."""
    x, B, codon = _dev(x, "x"), _dev(B, "B"), _dev(codon, "codon")
    state_row = _dev(state_row, "state_row", torch.int32)
    state_codon = _dev(state_codon, "state_codon", torch.int32)
    if x.dim() != 3:
        raise ValueError("x must have shape (b, L, s+5), got %s" % (tuple(x.shape),))
    b, L, w = x.shape
    s = w - 5
    rows, q, nc = B.shape[0], state_row.numel(), codon.shape[1]
    if B.shape[1] != s or tuple(codon.shape) != (2, nc, 64) or state_codon.numel() != q:
        raise ValueError("inconsistent emitter tables")
    return x, B, state_row, codon, state_codon, (b, L, s, rows, q, nc)


def _gene_emissions(name, x, B, state_row, codon, state_codon, free_value, add, n_mass):
    x, B, state_row, codon, state_codon, (b, L, s, rows, q, nc) = _emitter_args(x, B, state_row, codon, state_codon)
    with torch.cuda.device(x.device):
        E = torch.empty((b, L, q), dtype=torch.float32, device=x.device)
        _check(getattr(lib(), name)(x.data_ptr(), b, L, s, B.data_ptr(), rows, state_row.data_ptr(),
                                    codon.data_ptr(), nc, state_codon.data_ptr(), q, float(free_value),
                                    float(add), int(n_mass), E.data_ptr(), _stream(x.device)))
    return E


def gene_emissions(x, B, state_row, codon, state_codon, free_value=1.0 / 4096.0, add=0.0, n_mass=1):
    """Fused GenePredHMMEmitter.forward for one model: x (b,L,s+5) -> E (b,L,q) fp32.
    B (rows,s) fp32, state_row (q) int32, codon (2,nc,64) fp32, state_codon (q) int32.  q <= 64, rows <= 32."""
    return _gene_emissions("hmm_gene_emissions", x, B, state_row, codon, state_codon, free_value, add, n_mass)


def gene_emissions_wide(x, B, state_row, codon, state_codon, free_value=1.0 / 4096.0, add=0.0, n_mass=1):
    """gene_emissions for q <= 256 states and rows <= 256 (hmm_gene_emissions_wide): the gene models of three to
    eighteen copies.  Same arguments, same values."""
    return _gene_emissions("hmm_gene_emissions_wide", x, B, state_row, codon, state_codon, free_value, add, n_mass)


def gene_emissions_routes_wide(q, rows):
    """The routing rule of the layer and of autograd.GeneEmissions: None = no fused kernel serves the shape, False =
    hmm_gene_emissions / _grad (q <= 64 and rows <= 32: what the 15- and 29-state models always used), True = the
    _wide pair."""
    if q <= 64 and rows <= 32:
        return False
    return True if max(q, rows) <= lib().hmm_gene_emissions_wide_max_states() else None


def _gene_emissions_grad(name, tag, x, B, state_row, codon, state_codon, dE, free_value, add, n_mass, want_dx, want_dB):
    x, B, state_row, codon, state_codon, (b, L, s, rows, q, nc) = _emitter_args(x, B, state_row, codon, state_codon)
    dE = _dev(dE, "dE")
    if tuple(dE.shape) != (b, L, q):
        raise ValueError("dE must have shape %s, got %s" % ((b, L, q), tuple(dE.shape)))
    if not (want_dx or want_dB):
        return None, None
    with torch.cuda.device(x.device):
        # at most 1024 x rows x s floats: no floor
        ws = _workspace(x.device, getattr(lib(), name + "_workspace_bytes")(b, L, s, rows, q), tag, floor=0)
        dx = torch.empty_like(x) if want_dx else None
        dB = torch.empty_like(B) if want_dB else None
        _check(getattr(lib(), name)(x.data_ptr(), b, L, s, B.data_ptr(), rows, state_row.data_ptr(),
                                    codon.data_ptr(), nc, state_codon.data_ptr(), q, float(free_value),
                                    float(add), int(n_mass), dE.data_ptr(),
                                    dx.data_ptr() if want_dx else None, dB.data_ptr() if want_dB else None,
                                    ws.data_ptr(), ws.numel(), _stream(x.device)))
    return dx, dB


def gene_emissions_grad(x, B, state_row, codon, state_codon, dE, free_value=1.0 / 4096.0, add=0.0, n_mass=1,
                        want_dx=True, want_dB=True):
    """Backward of gene_emissions (hmm_gene_emissions_grad): dE (b,L,q) = dL/dE -> (dx (b,L,s+5) | None,
    dB (rows,s) | None).  The five nucleotide columns of dx are exactly 0 (one-hot nucleotides are data); dB is
    written whole by the call and summed in a fixed order, so repeated calls are bit-identical.  The workspace
    (one (rows,s) partial per workgroup, at most 1024 of them) comes from the engine's cache under a key of its
    own per device and stream, so it never overwrites the routing records that exact_count() and its kin read
    from the recursions' workspace."""
    return _gene_emissions_grad("hmm_gene_emissions_grad", "emitter_grad", x, B, state_row, codon, state_codon, dE,
                                free_value, add, n_mass, want_dx, want_dB)


def gene_emissions_grad_wide(x, B, state_row, codon, state_codon, dE, free_value=1.0 / 4096.0, add=0.0, n_mass=1,
                             want_dx=True, want_dB=True):
    """gene_emissions_grad for q <= 256 states and rows <= 256 (hmm_gene_emissions_grad_wide).  Same arguments, same
    values; the workspace (at most 1024 partials and at most 16 MiB, whatever b L) has a cache key of its own."""
    return _gene_emissions_grad("hmm_gene_emissions_grad_wide", "emitter_grad_wide", x, B, state_row, codon,
                                state_codon, dE, free_value, add, n_mass, want_dx, want_dB)


def _embedding_args(x, col0, d, mean, inv_std, log_norm, state_row):
    """Validation shared by embedding_emissions and embedding_emissions_grad -> (the five tensors, col0, d,
    (b, L, w, rows, q))."""
    x, mean, inv_std, log_norm = _dev(x, "x"), _dev(mean, "mean"), _dev(inv_std, "inv_std"), _dev(log_norm, "log_norm")
    state_row = _dev(state_row, "state_row", torch.int32)
    if x.dim() != 3:
        raise ValueError("x must have shape (b, L, w), got %s" % (tuple(x.shape),))
    b, L, w = x.shape
    col0, d = int(col0), int(d)
    rows, q = mean.shape[0], state_row.numel()
    if col0 < 0 or d < 1 or col0 + d > w:
        raise ValueError("columns %d .. %d lie outside x's %d columns" % (col0, col0 + d - 1, w))
    if tuple(mean.shape) != (rows, d) or tuple(inv_std.shape) != (rows, d) or log_norm.numel() != rows:
        raise ValueError("inconsistent embedding tables")
    return x, mean, inv_std, log_norm, state_row, col0, d, (b, L, w, rows, q)


def _is_E(t, shape):
    return (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
            and tuple(t.shape) == shape)


def _embedding_emissions(name, x, col0, d, mean, inv_std, log_norm, state_row, E, inv_temperature, add):
    x, mean, inv_std, log_norm, state_row, col0, d, (b, L, w, rows, q) = _embedding_args(
        x, col0, d, mean, inv_std, log_norm, state_row)
    multiply = E is not None
    if multiply:
        if not _is_E(E, (b, L, q)):
            raise ValueError("E must be a contiguous fp32 device tensor of shape %s" % ((b, L, q),))
    with torch.cuda.device(x.device):
        if not multiply:
            E = torch.empty((b, L, q), dtype=torch.float32, device=x.device)
        _check(getattr(lib(), name)(x.data_ptr() + 4 * col0, w, b, L, d, mean.data_ptr(), inv_std.data_ptr(),
                                    log_norm.data_ptr(), rows, state_row.data_ptr(), q,
                                    float(inv_temperature), float(add), int(multiply), E.data_ptr(),
                                    _stream(x.device)))
    return E


def embedding_emissions(x, col0, d, mean, inv_std, log_norm, state_row, E=None, inv_temperature=1.0, add=0.0):
    """Embedding-emission factor (hmm_embedding_emissions): x (b,L,w) fp32 holds every position's embedding in
    columns col0 .. col0+d-1, read in place (no copy of the columns is made).  mean, inv_std (rows,d) fp32,
    log_norm (rows) fp32, state_row (q) int32.  f = exp(inv_temperature * log N(x; mean, 1/inv_std)) + add.
    With E (b,L,q) given, E *= f in place; otherwise a new E = f.  Returns E.  q <= 64, rows <= 32."""
    return _embedding_emissions("hmm_embedding_emissions", x, col0, d, mean, inv_std, log_norm, state_row, E,
                                inv_temperature, add)


def embedding_emissions_wide(x, col0, d, mean, inv_std, log_norm, state_row, E=None, inv_temperature=1.0, add=0.0):
    """embedding_emissions for q <= 256 states and rows <= 256 (hmm_embedding_emissions_wide): the gene models of
    three to eighteen copies.  Same arguments; where both apply, bit-identical values."""
    return _embedding_emissions("hmm_embedding_emissions_wide", x, col0, d, mean, inv_std, log_norm, state_row, E,
                                inv_temperature, add)


def embedding_emissions_routes_wide(q, rows):
    """The routing rule of the layer and of autograd.EmbeddingEmissions: None = no fused kernel serves the shape,
    False = hmm_embedding_emissions / _grad (q <= 64 and rows <= 32: what the 15- and 29-state models always used),
    True = the _wide pair."""
    if q <= 64 and rows <= 32:
        return False
    return True if max(q, rows) <= lib().hmm_embedding_emissions_wide_max_states() else None


def _embedding_emissions_grad(name, tag, limits, x, col0, d, mean, inv_std, log_norm, state_row, dE, E_in,
                              inv_temperature, add, want_dE_in, want_demb, want_tables, dx_out):
    x, mean, inv_std, log_norm, state_row, col0, d, (b, L, w, rows, q) = _embedding_args(
        x, col0, d, mean, inv_std, log_norm, state_row)
    if not _is_E(dE, (b, L, q)):
        raise ValueError("dE must be a contiguous fp32 device tensor of shape %s" % ((b, L, q),))
    if E_in is not None and not _is_E(E_in, (b, L, q)):
        raise ValueError("E_in must be a contiguous fp32 device tensor of shape %s" % ((b, L, q),))
    if dx_out is not None and not _is_E(dx_out, (b, L, w)):
        raise ValueError("dx_out must be a contiguous fp32 device tensor of shape %s" % ((b, L, w),))
    want_dE_in = bool(want_dE_in) and E_in is not None
    if not (want_dE_in or want_demb or want_tables):
        return None, None, None, None, None
    need = getattr(lib(), name + "_workspace_bytes")(b, L, d, rows, q)
    if need == 0:
        raise ValueError("%s covers %s, d <= %d (got q = %d, rows = %d, d = %d)"
                         % (name, limits, lib().hmm_embedding_emissions_grad_max_dim(), q, rows, d))
    with torch.cuda.device(x.device):
        ws = _workspace(x.device, need, tag, floor=0)
        dE_in = torch.empty_like(dE) if want_dE_in else None
        demb, demb_ptr, ldd = None, None, 0
        if want_demb and dx_out is not None:
            demb, demb_ptr, ldd = dx_out, dx_out.data_ptr() + 4 * col0, w
        elif want_demb:
            demb = torch.empty((b, L, d), dtype=torch.float32, device=x.device)
            demb_ptr, ldd = demb.data_ptr(), d
        dmean = torch.empty_like(mean) if want_tables else None
        dinv_std = torch.empty_like(inv_std) if want_tables else None
        dlog_norm = torch.empty_like(log_norm) if want_tables else None
        _check(getattr(lib(), name)(
            x.data_ptr() + 4 * col0, w, b, L, d, mean.data_ptr(), inv_std.data_ptr(), log_norm.data_ptr(), rows,
            state_row.data_ptr(), q, float(inv_temperature), float(add),
            E_in.data_ptr() if E_in is not None else None, dE.data_ptr(), dE_in.data_ptr() if want_dE_in else None,
            demb_ptr, ldd, dmean.data_ptr() if want_tables else None, dinv_std.data_ptr() if want_tables else None,
            dlog_norm.data_ptr() if want_tables else None, ws.data_ptr(), ws.numel(), _stream(x.device)))
    return dE_in, demb, dmean, dinv_std, dlog_norm


def embedding_emissions_grad(x, col0, d, mean, inv_std, log_norm, state_row, dE, E_in=None, inv_temperature=1.0,
                             add=0.0, want_dE_in=True, want_demb=True, want_tables=True, dx_out=None):
    """Backward of embedding_emissions (hmm_embedding_emissions_grad): dE (b,L,q) = dL/dE_out ->
    (dE_in (b,L,q) | None, demb | None, dmean (rows,d) | None, dinv_std (rows,d) | None, dlog_norm (rows) | None).
    x, col0, d and the tables as for embedding_emissions; E_in (b,L,q) is the tensor the forward multiplied
    into (None: the forward wrote E = f, and there is no dE_in).  demb is a new (b,L,d) tensor, or, with dx_out
    (a contiguous fp32 tensor of x's shape) given, dx_out itself with its columns col0 .. col0+d-1 overwritten
    in place and every other column left as it was.  The three table gradients are written whole and summed in
    a fixed order: repeated calls, and calls for a subset of the outputs, are bit-identical.  The workspace
    (W (b L, rows) and at most 16 MiB of workgroup partials) comes from the engine's cache under a key of its
    own per device and stream."""
    return _embedding_emissions_grad("hmm_embedding_emissions_grad", "embedding_grad", "q <= 64, rows <= 32", x, col0,
                                     d, mean, inv_std, log_norm, state_row, dE, E_in, inv_temperature, add,
                                     want_dE_in, want_demb, want_tables, dx_out)


def embedding_emissions_grad_wide(x, col0, d, mean, inv_std, log_norm, state_row, dE, E_in=None, inv_temperature=1.0,
                                  add=0.0, want_dE_in=True, want_demb=True, want_tables=True, dx_out=None):
    """embedding_emissions_grad for q <= 256 states and rows <= 256 (hmm_embedding_emissions_grad_wide).  Same
    arguments, same formulas; the workspace (W (b L, rows) and at most 16 MiB of partials) has a cache key of its
    own."""
    return _embedding_emissions_grad("hmm_embedding_emissions_grad_wide", "embedding_grad_wide",
                                     "q <= 256, rows <= 256", x, col0, d, mean, inv_std, log_norm, state_row, dE, E_in,
                                     inv_temperature, add, want_dE_in, want_demb, want_tables, dx_out)


def _nucleotide_args(x, col0, P, state_nuc):
    """Validation shared by nucleotide_emissions and nucleotide_emissions_grad -> (the three tensors, col0,
    (b, L, w, rows, q))."""
    x, P = _dev(x, "x"), _dev(P, "P")
    state_nuc = _dev(state_nuc, "state_nuc", torch.int32)
    if x.dim() != 3:
        raise ValueError("x must have shape (b, L, w), got %s" % (tuple(x.shape),))
    b, L, w = x.shape
    col0 = int(col0)
    if col0 < 0 or col0 + 5 > w:
        raise ValueError("columns %d .. %d lie outside x's %d columns" % (col0, col0 + 4, w))
    if P.dim() != 2 or P.shape[1] != 4:
        raise ValueError("P must have shape (rows, 4), got %s" % (tuple(P.shape),))
    rows, q = P.shape[0], state_nuc.numel()
    limit = lib().hmm_nucleotide_emissions_max_states()
    if not (1 <= q <= limit and 1 <= rows <= limit):
        raise ValueError("hmm_nucleotide_emissions covers 1 <= q, rows <= %d (got q = %d, rows = %d)" % (limit, q, rows))
    return x, P, state_nuc, col0, (b, L, w, rows, q)


def nucleotide_emissions(x, col0, P, state_nuc, E=None, free_value=0.25):
    """Trainable nucleotide factor (hmm_nucleotide_emissions): x (b,L,w) fp32 holds every position's five nucleotide
    floats A,C,G,T,N in columns col0 .. col0+4, read in place (no copy of the columns is made).  P (rows,4) fp32,
    state_nuc (q) int32: the row of P feeding state j, or < 0 for a free state (f = free_value).
    f = sum_a (x[col0+a] + x[col0+4] / 4) P[state_nuc[j]][a].  With E (b,L,q) given, E *= f in place; otherwise a
    new E = f.  Returns E.  q <= 256, rows <= 256."""
    x, P, state_nuc, col0, (b, L, w, rows, q) = _nucleotide_args(x, col0, P, state_nuc)
    multiply = E is not None
    if multiply and not _is_E(E, (b, L, q)):
        raise ValueError("E must be a contiguous fp32 device tensor of shape %s" % ((b, L, q),))
    with torch.cuda.device(x.device):
        if not multiply:
            E = torch.empty((b, L, q), dtype=torch.float32, device=x.device)
        _check(lib().hmm_nucleotide_emissions(x.data_ptr() + 4 * col0, w, b, L, P.data_ptr(), rows,
                                              state_nuc.data_ptr(), q, float(free_value), int(multiply),
                                              E.data_ptr(), _stream(x.device)))
    return E


def nucleotide_emissions_grad(x, col0, P, state_nuc, dE, E_in=None, free_value=0.25, want_dE_in=True, want_dP=True):
    """Backward of nucleotide_emissions (hmm_nucleotide_emissions_grad): dE (b,L,q) = dL/dE_out ->
    (dE_in (b,L,q) | None, dP (rows,4) | None).  x, col0, P and state_nuc as for nucleotide_emissions; E_in (b,L,q)
    is the tensor the forward multiplied into (None: the forward wrote E = f, E_in counts as ones).  There is no
    gradient for x: nucleotides are data.  dP is written whole and summed in a fixed order: repeated calls, and
    calls for either output alone, are bit-identical.  The workspace (one (rows,4) partial per workgroup, at most
    1024 of them) comes from the engine's cache under a key of its own per device and stream."""
    x, P, state_nuc, col0, (b, L, w, rows, q) = _nucleotide_args(x, col0, P, state_nuc)
    if not _is_E(dE, (b, L, q)):
        raise ValueError("dE must be a contiguous fp32 device tensor of shape %s" % ((b, L, q),))
    if E_in is not None and not _is_E(E_in, (b, L, q)):
        raise ValueError("E_in must be a contiguous fp32 device tensor of shape %s" % ((b, L, q),))
    if not (want_dE_in or want_dP):
        return None, None
    with torch.cuda.device(x.device):
        # at most 1024 x rows x 4 floats: no floor
        ws = _workspace(x.device, lib().hmm_nucleotide_emissions_grad_workspace_bytes(b, L, rows, q),
                        "nucleotide_grad", floor=0)
        dE_in = torch.empty_like(dE) if want_dE_in else None
        dP = torch.empty_like(P) if want_dP else None
        _check(lib().hmm_nucleotide_emissions_grad(
            x.data_ptr() + 4 * col0, w, b, L, P.data_ptr(), rows, state_nuc.data_ptr(), q, float(free_value),
            E_in.data_ptr() if E_in is not None else None, dE.data_ptr(), dE_in.data_ptr() if want_dE_in else None,
            dP.data_ptr() if want_dP else None, ws.data_ptr(), ws.numel(), _stream(x.device)))
    return dE_in, dP


def _viterbi(name, logA, logpi, logE):
    """The body of viterbi / viterbi_scan / viterbi_large: hmm_<name> with the workspace cached under `name`."""
    logA, logpi, logE = _dev(logA, "logA"), _dev(logpi, "logpi"), _dev(logE, "logE")
    logA, logpi, dims = _shapes(logA, logE, logpi)
    k, b, L, q = dims
    if name == "viterbi":
        if q > lib().hmm_viterbi_max_states():
            name = "viterbi_large"
        elif q > lib().hmm_scan_max_states() and lib().hmm_viterbi_scan_pays(*dims):
            name = "viterbi_scan"
    limit = getattr(lib(), "hmm_%s_max_states" % name)()
    if q > limit:
        raise ValueError("%s covers q <= %d states, got %d" % (name, limit, q))
    with torch.cuda.device(logE.device):
        ws = _workspace(logE.device, getattr(lib(), "hmm_%s_workspace_bytes" % name)(*dims), name)
        path = torch.empty((k, b, L), dtype=torch.int32, device=logE.device)
        score = torch.empty((k, b), dtype=torch.float64, device=logE.device)
        _check(getattr(lib(), "hmm_" + name)(logA.data_ptr(), logpi.data_ptr(), logE.data_ptr(), *dims,
                                             path.data_ptr(), score.data_ptr(), ws.data_ptr(), ws.numel(),
                                             _stream(logE.device)))
    return path, score


def viterbi(logA, logpi, logE):
    """Most probable state paths.  logA (k,q,q), logpi (k,q), logE (k,b,L,q) fp32 log-probabilities
    (-inf allowed: anything below -1024 counts as -1024).  -> (path (k,b,L) int32, score (k,b) fp64).
    Scores are Q16 fixed point, so the result is bit-identical to the serial recursion
    (oracle/viterbi.py); ties take the lowest state index.  q <= 64 runs hmm_viterbi — or, for 17..64 states
    and the few long sequences where hmm_viterbi_scan_pays says so, viterbi_scan: bit-identical results, only
    faster —, larger models viterbi_large (hmm_viterbi_large)."""
    return _viterbi("viterbi", logA, logpi, logE)


def viterbi_scan(logA, logpi, logE):
    """viterbi() through hmm_viterbi_scan, the time-parallel chunk scan for 1 <= q <= 64 (same arguments, results
    and semantics): what few, long sequences of the 17..64-state models want.  OPT_CHUNK forces the chunk length,
    OPT_SCAN2 = 0 the single-level chunk scans, OPT_FORCE_DENSE = 1 the all-candidates reduce."""
    return _viterbi("viterbi_scan", logA, logpi, logE)


def viterbi_large(logA, logpi, logE):
    """viterbi() through hmm_viterbi_large, for any 1 <= q <= 4096 (same arguments, results and semantics;
    the walk / tile evaluation is chosen by q or by OPT_VLARGE)."""
    return _viterbi("viterbi_large", logA, logpi, logE)


def loglik_partials(loglik, weights=None):
    """(k,b) fp64 loglik [, (k,b) fp32 weights] -> (k,2) fp64: (sum w*loglik, sum w) per model."""
    loglik = _dev(loglik, "loglik", torch.float64)
    k, b = loglik.shape
    if weights is not None:
        weights = _dev(weights, "weights")
        if tuple(weights.shape) != (k, b):
            raise ValueError("weights must have shape %s" % ((k, b),))
    with torch.cuda.device(loglik.device):
        part = torch.empty((k, 2), dtype=torch.float64, device=loglik.device)
        _check(lib().hmm_loglik_partials(loglik.data_ptr(),
                                         weights.data_ptr() if weights is not None else None,
                                         k, b, part.data_ptr(), _stream(loglik.device)))
    return part


def _seqshard_ws(dims, R, device):
    need = lib().hmm_seqshard_workspace_bytes(*dims, int(R))
    if need == 0:
        raise ValueError("sequence-sharded calls cover q <= %d states" % lib().hmm_scan_max_states())
    return _workspace(device, need, "seqshard")


def seqshard_reduce(A, E_slab, seq_start, R, eps=EPS):
    """Step 1 of the sequence-sharded posterior (include/hmm_engine.h): this rank's time slab E_slab
    (k,b,Ls,q) -> its operator per sequence, (k,b,16,16) fp32 and (k,b,16) int32 exponents.  The chunk
    operators stay in this device's "seqshard" workspace for seqshard_posterior."""
    A, E = _dev(A, "A"), _dev(E_slab, "E_slab")
    A, _, dims = _shapes(A, E)
    k, b = dims[:2]
    with torch.cuda.device(E.device):
        ws = _seqshard_ws(dims, R, E.device)
        op = torch.empty((k, b, 16, 16), dtype=torch.float32, device=E.device)
        ex = torch.empty((k, b, 16), dtype=torch.int32, device=E.device)
        _check(lib().hmm_seqshard_reduce(A.data_ptr(), E.data_ptr(), *dims, eps, int(bool(seq_start)), int(R),
                                         op.data_ptr(), ex.data_ptr(), ws.data_ptr(), ws.numel(), _stream(E.device)))
    return op, ex


def seqshard_posterior(A, pi, E_slab, all_ops, all_exps, r, mode=POST_PROB, eps=EPS):
    """Step 3: all_ops (k,b,R,16,16) / all_exps (k,b,R,16) = every rank's slab operators in time order;
    -> (out (k,b,Ls,q), loglik (k,b) fp64 of the whole sequences, phi (k,b) fp32: this slab's share of
    the floor-transition bound)."""
    A, pi, E = _dev(A, "A"), _dev(pi, "pi"), _dev(E_slab, "E_slab")
    all_ops, all_exps = _dev(all_ops, "all_ops", align=16), _dev(all_exps, "all_exps", torch.int32)
    A, pi, dims = _shapes(A, E, pi)
    k, b = dims[:2]
    R = all_ops.shape[2]
    if tuple(all_ops.shape) != (k, b, R, 16, 16) or tuple(all_exps.shape) != (k, b, R, 16):
        raise ValueError("all_ops / all_exps must have shapes (k,b,R,16,16) / (k,b,R,16)")
    with torch.cuda.device(E.device):
        ws = _seqshard_ws(dims, R, E.device)
        out = torch.empty_like(E)
        ll = torch.empty((k, b), dtype=torch.float64, device=E.device)
        phi = torch.empty((k, b), dtype=torch.float32, device=E.device)
        _check(lib().hmm_seqshard_posterior(A.data_ptr(), pi.data_ptr(), E.data_ptr(), *dims, eps, int(r == 0),
                                            all_ops.data_ptr(), all_exps.data_ptr(), int(R), int(r), int(mode),
                                            out.data_ptr(), ll.data_ptr(), phi.data_ptr(), ws.data_ptr(), ws.numel(),
                                            _stream(E.device)))
    return out, ll, phi


def _seqshard_viterbi_ws(dims, R, device):
    q = dims[3]
    if q > lib().hmm_seqshard_viterbi_max_states():
        raise ValueError("sequence-sharded Viterbi covers q <= %d states, got %d"
                         % (lib().hmm_seqshard_viterbi_max_states(), q))
    need = lib().hmm_seqshard_viterbi_workspace_bytes(*dims, int(R))
    if need == 0:
        raise ValueError("bad sequence-sharded Viterbi call: (k, b, Ls, q) = %s, R = %d" % (tuple(dims), R))
    return _workspace(device, need, "seqshard_viterbi")


def _log_model(logA, logpi, logE_slab):
    logA, logpi, logE = _dev(logA, "logA"), _dev(logpi, "logpi"), _dev(logE_slab, "logE_slab")
    logA, logpi, dims = _shapes(logA, logE, logpi)
    return logA.contiguous(), logpi.contiguous(), logE, dims


def seqshard_viterbi_reduce(logA, logpi, logE_slab, seq_start, R):
    """Step 1 of the sequence-sharded Viterbi (include/hmm_engine.h): this rank's time slab logE_slab (k,b,Ls,q) of
    log-probabilities -> its max-plus operator per sequence, slab_vop (k,b,16,16) int32 (every column has maximum 0)
    and slab_vbase (k,b,16) int64.  The chunk operators stay in this device's "seqshard_viterbi" workspace (one per
    stream) for seqshard_viterbi_apply."""
    logA, logpi, logE, dims = _log_model(logA, logpi, logE_slab)
    k, b = dims[:2]
    with torch.cuda.device(logE.device):
        ws = _seqshard_viterbi_ws(dims, R, logE.device)
        vop = torch.empty((k, b, 16, 16), dtype=torch.int32, device=logE.device)
        vbase = torch.empty((k, b, 16), dtype=torch.int64, device=logE.device)
        _check(lib().hmm_seqshard_viterbi_reduce(logA.data_ptr(), logpi.data_ptr(), logE.data_ptr(), *dims,
                                                 int(bool(seq_start)), int(R), vop.data_ptr(), vbase.data_ptr(),
                                                 ws.data_ptr(), ws.numel(), _stream(logE.device)))
    return vop, vbase


def seqshard_viterbi_apply(logA, logpi, logE_slab, all_vops, all_vbases, r):
    """Step 3: all_vops (k,b,R,16,16) int32 / all_vbases (k,b,R,16) int64 = every rank's slab operators in time order
    -> (origin (k,b,16) uint8: the state before the slab of the best path into every state at the slab's last
    position; final_state (k,b) int32 and score (k,b) fp64 of the WHOLE sequences, the same on every rank).  The
    backpointers stay in the workspace for seqshard_viterbi_path."""
    logA, logpi, logE, dims = _log_model(logA, logpi, logE_slab)
    all_vops, all_vbases = _dev(all_vops, "all_vops", torch.int32, align=16), _dev(all_vbases, "all_vbases", torch.int64)
    k, b = dims[:2]
    R = all_vops.shape[2] if all_vops.dim() == 5 else 0
    if tuple(all_vops.shape) != (k, b, R, 16, 16) or tuple(all_vbases.shape) != (k, b, R, 16):
        raise ValueError("all_vops / all_vbases must have shapes (k,b,R,16,16) / (k,b,R,16)")
    with torch.cuda.device(logE.device):
        ws = _seqshard_viterbi_ws(dims, R, logE.device)
        origin = torch.empty((k, b, 16), dtype=torch.uint8, device=logE.device)
        final_state = torch.empty((k, b), dtype=torch.int32, device=logE.device)
        score = torch.empty((k, b), dtype=torch.float64, device=logE.device)
        _check(lib().hmm_seqshard_viterbi_apply(logA.data_ptr(), logpi.data_ptr(), logE.data_ptr(), *dims, int(r == 0),
                                                all_vops.data_ptr(), all_vbases.data_ptr(), int(R), int(r),
                                                origin.data_ptr(), final_state.data_ptr(), score.data_ptr(),
                                                ws.data_ptr(), ws.numel(), _stream(logE.device)))
    return origin, final_state, score


def seqshard_viterbi_path(dims, all_origins, final_state, r):
    """Step 5: dims = (k, b, Ls, q) of this rank's slab, all_origins (k,b,R,16) uint8 = every rank's origin in time
    order, final_state (k,b) int32 -> path (k,b,Ls) int32, this slab's piece of the most probable path."""
    k, b, Ls, q = (int(d) for d in dims)
    all_origins = _dev(all_origins, "all_origins", torch.uint8)
    final_state = _dev(final_state, "final_state", torch.int32)
    R = all_origins.shape[2] if all_origins.dim() == 4 else 0
    if tuple(all_origins.shape) != (k, b, R, 16) or tuple(final_state.shape) != (k, b):
        raise ValueError("all_origins / final_state must have shapes (k,b,R,16) / (k,b)")
    device = all_origins.device
    with torch.cuda.device(device):
        ws = _seqshard_viterbi_ws((k, b, Ls, q), R, device)
        path = torch.empty((k, b, Ls), dtype=torch.int32, device=device)
        _check(lib().hmm_seqshard_viterbi_path(k, b, Ls, q, all_origins.data_ptr(), final_state.data_ptr(), int(R),
                                               int(r), path.data_ptr(), ws.data_ptr(), ws.numel(), _stream(device)))
    return path


def loglik_allreduce(comm, partial):
    """In-place all-reduce(sum) of the (k,2) fp64 partials over a raw RCCL communicator (an ncclComm_t as an
    integer / ctypes pointer) created by the caller — the C-ABI route for hosts without
    torch.distributed; hmm_layer_amd.distributed uses torch's process group instead."""
    partial = _dev(partial, "partial", torch.float64)
    if partial.dim() != 2 or partial.shape[1] != 2:
        raise ValueError("partial must have shape (k, 2)")
    with torch.cuda.device(partial.device):
        _check(lib().hmm_loglik_allreduce(ctypes.c_void_p(int(comm) if not isinstance(comm, ctypes.c_void_p) else comm.value),
                                          partial.data_ptr(), partial.shape[0], _stream(partial.device)))
    return partial


def _loglik_grad(name, limit, A, pi, E, grad_loglik, eps):
    """The body of loglik_grad / loglik_grad_scan / loglik_grad_large: hmm_<name>, covering q <= hmm_<limit>().
    loglik_grad_scan keeps its workspace under a tag of its own."""
    A, pi, E = _dev(A, "A"), _dev(pi, "pi"), _dev(E, "E")
    A, pi, dims = _shapes(A, E, pi)
    k, b, L, q = dims
    if name == "loglik_grad" and lib().hmm_scan_max_states() < q <= lib().hmm_loglik_grad_scan_max_states() \
            and lib().hmm_loglik_grad_scan_pays(*dims):
        name, limit = "loglik_grad_scan", "hmm_loglik_grad_scan_max_states"
    limit = getattr(lib(), limit)()
    if q > limit:
        raise ValueError("%s covers q <= %d states, got %d" % (name, limit, q))
    if grad_loglik is not None:
        grad_loglik = _dev(grad_loglik, "grad_loglik")
        if tuple(grad_loglik.shape) != (k, b):
            raise ValueError("grad_loglik must have shape %s" % ((k, b),))
    with torch.cuda.device(E.device):
        need = getattr(lib(), "hmm_%s_workspace_bytes" % name)(*dims)
        if name == "loglik_grad_scan" and need == 0:
            raise ValueError("loglik_grad_scan does not support the shape (k, b, L, q) = %s" % (dims,))
        ws = _workspace(E.device, need, "loglik_grad_scan" if name == "loglik_grad_scan" else None)
        dA = torch.empty((k, q, q), dtype=torch.float32, device=E.device)
        dpi = torch.empty((k, q), dtype=torch.float32, device=E.device)
        dE = torch.empty_like(E)
        ll = torch.empty((k, b), dtype=torch.float64, device=E.device)
        _check(getattr(lib(), "hmm_" + name)(A.data_ptr(), pi.data_ptr(), E.data_ptr(), *dims, eps,
                                             grad_loglik.data_ptr() if grad_loglik is not None else None,
                                             dA.data_ptr(), dpi.data_ptr(), dE.data_ptr(), ll.data_ptr(),
                                             ws.data_ptr(), ws.numel(), _stream(E.device)))
    return dA, dpi, dE, ll


def loglik_grad(A, pi, E, grad_loglik=None, eps=EPS):
    """Gradients of sum_{m,s} grad_loglik[m,s] * loglik[m,s] -> (dA (k,q,q), dpi (k,q), dE (k,b,L,q), loglik (k,b) fp64).

    What autograd through the reference's time loop (hmm_layer/BaseRNN.py:217-227) computes, from
    one forward-backward pass.  17..64 states: through loglik_grad_scan where hmm_loglik_grad_scan_pays says so."""
    return _loglik_grad("loglik_grad", "hmm_grad_max_states", A, pi, E, grad_loglik, eps)


def loglik_grad_scan(A, pi, E, grad_loglik=None, eps=EPS):
    """loglik_grad() through hmm_loglik_grad_scan, per chunk of the scan plan for 1 <= q <= 64 (same arguments,
    results and semantics): what few, long sequences of the 17..64-state models want.  OPT_CHUNK forces the chunk
    length, OPT_PGCHUNK = 2 serves every sequence per chunk (tests); loglik_grad_scan_serial_count() tells how many
    sequences the whole-sequence sweeps redid."""
    return _loglik_grad("loglik_grad_scan", "hmm_loglik_grad_scan_max_states", A, pi, E, grad_loglik, eps)


def loglik_grad_large(A, pi, E, grad_loglik=None, eps=EPS):
    """loglik_grad() through hmm_loglik_grad_large, for any 1 <= q <= 4096 (same arguments, results and
    semantics; the walk / GEMM evaluation is chosen by q or by OPT_GLARGE)."""
    return _loglik_grad("loglik_grad_large", "hmm_loglik_grad_large_max_states", A, pi, E, grad_loglik, eps)


GRAD_WALK_TAG = "loglik_grad_walk"   # loglik_grad_walk()'s workspace: loglik_grad_walk_refused() reads its counter


def loglik_grad_walk(A, pi, E, grad_loglik=None, eps=EPS, want_grads=True, check=True):
    """-> (dA, dpi, dE, loglik (k,b) fp64) by the per-sequence walk with the sparse step for 65..256 states
    (hmm_loglik_grad_walk), or (None, None, None, loglik) with want_grads=False: the log-likelihood alone, bit for bit
    the gradient call's.  dE and dpi are loglik_grad_large()'s; dA holds the same derivative wherever A != 0 and an
    exact 0 wherever A == 0 (a matrix scattered from per-edge parameters never reads those).  A model with more than
    two states above degree 8 is refused on the device (NaN in all its outputs): with check=True the call reads the
    refusal counter (one synchronisation) and raises EngineError.  Raises ValueError outside 65..256 states."""
    lo, hi = lib().hmm_loglik_grad_walk_min_states(), lib().hmm_loglik_grad_walk_max_states()
    if torch.is_tensor(E) and E.dim() == 4 and not lo <= E.shape[3] <= hi:     # (before the device is asked for)
        raise ValueError("loglik_grad_walk serves %d..%d states, got q = %d" % (lo, hi, E.shape[3]))
    A, pi, E = _dev(A, "A"), _dev(pi, "pi"), _dev(E, "E")
    A, pi, dims = _shapes(A, E, pi)
    k, b, L, q = dims
    if grad_loglik is not None:
        grad_loglik = _dev(grad_loglik, "grad_loglik")
        if tuple(grad_loglik.shape) != (k, b):
            raise ValueError("grad_loglik must have shape %s" % ((k, b),))
    with torch.cuda.device(E.device):
        ws = _workspace(E.device, lib().hmm_loglik_grad_walk_workspace_bytes(*dims), GRAD_WALK_TAG)
        dA = dpi = dE = None
        if want_grads:
            dA = torch.empty((k, q, q), dtype=torch.float32, device=E.device)
            dpi = torch.empty((k, q), dtype=torch.float32, device=E.device)
            dE = torch.empty_like(E)
        ll = torch.empty((k, b), dtype=torch.float64, device=E.device)
        _check(lib().hmm_loglik_grad_walk(A.data_ptr(), pi.data_ptr(), E.data_ptr(), *dims, eps,
                                          grad_loglik.data_ptr() if grad_loglik is not None else None,
                                          *(t.data_ptr() if t is not None else None for t in (dA, dpi, dE)),
                                          ll.data_ptr(), ws.data_ptr(), ws.numel(), _stream(E.device)))
        if check:
            n = loglik_grad_walk_refused(dims, E.device)
            if n:
                raise EngineError("loglik_grad_walk: %d of %d models have more than two states above degree 8 and "
                                  "were refused (their outputs are NaN)" % (n, k))
    return dA, dpi, dE, ll


def loglik_grad_walk_refused(dims, device=None):
    """How many of the k models of the LAST loglik_grad_walk call with shape `dims` on this device and stream were
    refused (synchronises)."""
    return posterior_grad_serial_count(dims, device, _fn="hmm_loglik_grad_walk_refused", _tag=GRAD_WALK_TAG)


def _posterior_grad(name, A, pi, E, grad_out, mode, eps):
    """The body of posterior_grad / posterior_grad_scan / posterior_grad_large: hmm_<name>, covering
    q <= hmm_<name>_max_states().  posterior_grad_scan keeps its workspace under a tag of its own."""
    if int(mode) not in (POST_PROB, POST_LOG):
        raise ValueError("%s supports mode POST_PROB or POST_LOG" % name)
    A, pi, E, grad_out = _dev(A, "A"), _dev(pi, "pi"), _dev(E, "E"), _dev(grad_out, "grad_out")
    A, pi, dims = _shapes(A, E, pi)
    k, b, L, q = dims
    if name == "posterior_grad" and lib().hmm_scan_max_states() < q <= lib().hmm_posterior_grad_scan_max_states() \
            and lib().hmm_posterior_grad_scan_pays(*dims):
        name = "posterior_grad_scan"
    limit = getattr(lib(), "hmm_%s_max_states" % name)()
    if q > limit:
        raise ValueError("%s covers q <= %d states, got %d" % (name, limit, q))
    if grad_out.shape != E.shape:
        raise ValueError("grad_out must be shaped like E")
    with torch.cuda.device(E.device):
        need = getattr(lib(), "hmm_%s_workspace_bytes" % name)(*dims)
        if name == "posterior_grad_scan" and need == 0:
            raise ValueError("posterior_grad_scan does not support the shape (k, b, L, q) = %s" % (dims,))
        ws = _workspace(E.device, need, "posterior_grad_scan" if name == "posterior_grad_scan" else None)
        dA = torch.empty((k, q, q), dtype=torch.float32, device=E.device)
        dpi = torch.empty((k, q), dtype=torch.float32, device=E.device)
        dE = torch.empty_like(E)
        _check(getattr(lib(), "hmm_" + name)(A.data_ptr(), pi.data_ptr(), E.data_ptr(), *dims, eps, int(mode),
                                             grad_out.data_ptr(), dA.data_ptr(), dpi.data_ptr(), dE.data_ptr(),
                                             ws.data_ptr(), ws.numel(), _stream(E.device)))
    return dA, dpi, dE


def posterior_grad(A, pi, E, grad_out, mode=POST_LOG, eps=EPS):
    """Gradients of <grad_out, out> with out = posterior(A, pi, E, mode) -> (dA (k,q,q), dpi (k,q), dE (k,b,L,q)).

    What autograd through the reference's _state_posterior_log_probs_impl loops computes
    (hmm_layer/MsaHMMLayer.py:422-521); mode POST_PROB or POST_LOG.  17..64 states: through posterior_grad_scan where
    hmm_posterior_grad_scan_pays says so."""
    return _posterior_grad("posterior_grad", A, pi, E, grad_out, mode, eps)


def posterior_grad_scan(A, pi, E, grad_out, mode=POST_LOG, eps=EPS):
    """posterior_grad() through hmm_posterior_grad_scan, per chunk of the scan plan for 1 <= q <= 64 (same arguments,
    results and semantics): what few, long sequences of the 17..64-state models want.  OPT_CHUNK forces the chunk
    length, OPT_PGCHUNK = 2 serves every sequence per chunk (tests); posterior_grad_scan_serial_count() tells how many
    sequences the whole-sequence sweeps redid."""
    return _posterior_grad("posterior_grad_scan", A, pi, E, grad_out, mode, eps)


def posterior_grad_large(A, pi, E, grad_out, mode=POST_LOG, eps=EPS):
    """posterior_grad() through hmm_posterior_grad_large, for any 1 <= q <= 4096 (same arguments, results and
    semantics; the walk / GEMM evaluation is chosen by q or by OPT_GLARGE).  POST_LOG_NO_LL is not a mode of
    this call: the autograd node composes it with loglik_grad_large."""
    return _posterior_grad("posterior_grad_large", A, pi, E, grad_out, mode, eps)


POSTGRAD_WALK_TAG = "posterior_grad_walk"   # posterior_grad_walk()'s workspace: posterior_grad_walk_refused() reads its counter


def posterior_grad_walk(A, pi, E, grad_out, mode=POST_LOG, eps=EPS, check=True):
    """posterior_grad() -> (dA, dpi, dE) by the per-sequence walk with the sparse step for 65..256 states
    (hmm_posterior_grad_walk).  dE and dpi are posterior_grad_large()'s; dA holds the same derivative wherever A != 0
    and an exact 0 wherever A == 0 (a matrix scattered from per-edge parameters never reads those).  A model with more
    than two states above degree 8 is refused on the device (NaN in all its outputs): with check=True the call reads
    the refusal counter (one synchronisation) and raises EngineError.  Raises ValueError outside 65..256 states and
    for a mode other than POST_PROB / POST_LOG (POST_LOG_NO_LL is composed by the autograd node)."""
    lo, hi = lib().hmm_posterior_grad_walk_min_states(), lib().hmm_posterior_grad_walk_max_states()
    if torch.is_tensor(E) and E.dim() == 4 and not lo <= E.shape[3] <= hi:     # (before the device is asked for)
        raise ValueError("posterior_grad_walk serves %d..%d states, got q = %d" % (lo, hi, E.shape[3]))
    if int(mode) not in (POST_PROB, POST_LOG):
        raise ValueError("posterior_grad_walk supports mode POST_PROB or POST_LOG")
    A, pi, E, grad_out = _dev(A, "A"), _dev(pi, "pi"), _dev(E, "E"), _dev(grad_out, "grad_out")
    A, pi, dims = _shapes(A, E, pi)
    k, b, L, q = dims
    if grad_out.shape != E.shape:
        raise ValueError("grad_out must be shaped like E")
    with torch.cuda.device(E.device):
        ws = _workspace(E.device, lib().hmm_posterior_grad_walk_workspace_bytes(*dims), POSTGRAD_WALK_TAG)
        dA = torch.empty((k, q, q), dtype=torch.float32, device=E.device)
        dpi = torch.empty((k, q), dtype=torch.float32, device=E.device)
        dE = torch.empty_like(E)
        _check(lib().hmm_posterior_grad_walk(A.data_ptr(), pi.data_ptr(), E.data_ptr(), *dims, eps, int(mode),
                                             grad_out.data_ptr(), dA.data_ptr(), dpi.data_ptr(), dE.data_ptr(),
                                             ws.data_ptr(), ws.numel(), _stream(E.device)))
        if check:
            n = posterior_grad_walk_refused(dims, E.device)
            if n:
                raise EngineError("posterior_grad_walk: %d of %d models have more than two states above degree 8 and "
                                  "were refused (their outputs are NaN)" % (n, k))
    return dA, dpi, dE


def posterior_grad_walk_refused(dims, device=None):
    """How many of the k models of the LAST posterior_grad_walk call with shape `dims` on this device and stream were
    refused (synchronises)."""
    return posterior_grad_serial_count(dims, device, _fn="hmm_posterior_grad_walk_refused", _tag=POSTGRAD_WALK_TAG)


CLASS_WALK_TAG = "class_posterior_walk"              # class_posterior_walk()'s workspace
CLASS_GRAD_WALK_TAG = "class_posterior_grad_walk"    # class_posterior_grad_walk()'s: its refusal counter is read from it


def _class_walk_args(name, E, state_class, num_classes):
    """Checks shared by class_posterior_walk and class_posterior_grad_walk, before the device is asked for
    -> (table as a ctypes array, C)."""
    lo, hi = lib().hmm_posterior_walk_min_states(), lib().hmm_posterior_walk_max_states()
    if not torch.is_tensor(E) or E.dim() != 4:
        raise ValueError("E must be a tensor of shape (k, b, L, q)")
    q = E.shape[3]
    if not lo <= q <= hi:
        raise ValueError("%s serves %d..%d states, got q = %d" % (name, lo, hi, q))
    if state_class is None:
        raise ValueError("%s needs a class table (state_class)" % name)
    table, C = class_table(state_class, num_classes, q)
    if C > 16:
        raise ValueError("at most 16 classes, got %d" % C)
    return (ctypes.c_int * q)(*table), C


def class_posterior_walk(A, pi, E, state_class, num_classes=None, eps=EPS, prob=True, log=False):
    """Class posteriors for 65..256 states by the per-sequence walk (hmm_class_posterior_walk)
    -> (prob (k,b,L,C) fp32 or None, log (k,b,L,C) fp32 or None, loglik (k,b) fp64): P_c[t] = the sum of the state
    posteriors of class c's states, with the bits posterior_decode's fused call compares; log = its log (-inf for a
    sum of 0).  The (k,b,L,q) tensor is not written (the workspace keeps a parking region of that size, as
    posterior_decode's).  state_class: a sequence or an integer tensor of q classes, at most 16 of them.  Raises
    ValueError outside 65..256 states, without a table, above 16 classes, or with neither output asked for."""
    tab, C = _class_walk_args("class_posterior_walk", E, state_class, num_classes)
    if not (prob or log):
        raise ValueError("class_posterior_walk: ask for prob, log or both")
    A, pi, E = _dev(A, "A"), _dev(pi, "pi"), _dev(E, "E")
    A, pi, dims = _shapes(A, E, pi)
    with torch.cuda.device(E.device):
        ws = _workspace(E.device, lib().hmm_class_posterior_walk_workspace_bytes(*dims), CLASS_WALK_TAG)
        P = torch.empty(dims[:3] + (C,), dtype=torch.float32, device=E.device) if prob else None
        Lg = torch.empty(dims[:3] + (C,), dtype=torch.float32, device=E.device) if log else None
        ll = torch.empty(dims[:2], dtype=torch.float64, device=E.device)
        _check(lib().hmm_class_posterior_walk(A.data_ptr(), pi.data_ptr(), E.data_ptr(), *dims, eps, tab, C,
                                              P.data_ptr() if prob else None, Lg.data_ptr() if log else None,
                                              ll.data_ptr(), ws.data_ptr(), ws.numel(), _stream(E.device)))
    return P, Lg, ll


def class_posterior_grad_walk(A, pi, E, state_class, num_classes, grad_out, class_prob=None, mode=POST_LOG, eps=EPS,
                              check=True):
    """Gradients of <grad_out, out> with out = the class posteriors (POST_PROB) or their logs (POST_LOG) of
    class_posterior_walk -> (dA (k,q,q), dpi (k,q), dE (k,b,L,q)) by hmm_class_posterior_grad_walk: grad_out is
    (k,b,L,C), and nothing of size (k,b,L,q) but dE and the walk's workspace is touched.  POST_PROB is
    posterior_grad_walk(POST_PROB) with grad_out[..., state_class], bit for bit; POST_LOG needs class_prob, the
    forward's prob, and passes nothing through a class whose posterior is 0.  dA has exact zeros wherever A == 0; a
    model outside the sparse rule is refused as in posterior_grad_walk (check=True: one synchronisation, EngineError)."""
    tab, C = _class_walk_args("class_posterior_grad_walk", E, state_class, num_classes)
    if int(mode) not in (POST_PROB, POST_LOG):
        raise ValueError("class_posterior_grad_walk supports mode POST_PROB or POST_LOG")
    if int(mode) == POST_LOG and class_prob is None:
        raise ValueError("class_posterior_grad_walk: POST_LOG needs class_prob (class_posterior_walk's prob)")
    A, pi, E, grad_out = _dev(A, "A"), _dev(pi, "pi"), _dev(E, "E"), _dev(grad_out, "grad_out")
    A, pi, dims = _shapes(A, E, pi)
    k, b, L, q = dims
    if tuple(grad_out.shape) != (k, b, L, C):
        raise ValueError("grad_out must have shape (k, b, L, C) = %s, got %s" % ((k, b, L, C), tuple(grad_out.shape)))
    if int(mode) == POST_LOG:
        class_prob = _dev(class_prob, "class_prob")
        if class_prob.shape != grad_out.shape:
            raise ValueError("class_prob must be shaped like grad_out")
    with torch.cuda.device(E.device):
        ws = _workspace(E.device, lib().hmm_class_posterior_grad_walk_workspace_bytes(*dims, C), CLASS_GRAD_WALK_TAG)
        dA = torch.empty((k, q, q), dtype=torch.float32, device=E.device)
        dpi = torch.empty((k, q), dtype=torch.float32, device=E.device)
        dE = torch.empty_like(E)
        _check(lib().hmm_class_posterior_grad_walk(
            A.data_ptr(), pi.data_ptr(), E.data_ptr(), *dims, eps, int(mode), tab, C,
            class_prob.data_ptr() if int(mode) == POST_LOG else None, grad_out.data_ptr(), dA.data_ptr(),
            dpi.data_ptr(), dE.data_ptr(), ws.data_ptr(), ws.numel(), _stream(E.device)))
        if check:
            n = class_posterior_grad_walk_refused(dims, E.device)
            if n:
                raise EngineError("class_posterior_grad_walk: %d of %d models have more than two states above degree "
                                  "8 and were refused (their outputs are NaN)" % (n, k))
    return dA, dpi, dE


def class_posterior_grad_walk_refused(dims, device=None):
    """How many of the k models of the LAST class_posterior_grad_walk call with shape `dims` on this device and stream
    were refused (synchronises): the workspace begins with hmm_posterior_grad_walk's layout."""
    return posterior_grad_serial_count(dims, device, _fn="hmm_posterior_grad_walk_refused", _tag=CLASS_GRAD_WALK_TAG)


CLASS_TAG = "class_posterior"              # class_posterior()'s workspace: exact_count(OP_POSTERIOR, ..., tag=CLASS_TAG) reads it
CLASS_GRAD_TAG = "class_posterior_grad"    # class_posterior_grad()'s: class_posterior_grad_serial_count() reads it
CLASS_MAX_STATES = 16                      # hmm_class_posterior_max_states(), known without the library


def _class_args(name, E, state_class, num_classes):
    """Checks shared by class_posterior and class_posterior_grad, before the device is asked for
    -> (table as a ctypes array, C)."""
    if not torch.is_tensor(E) or E.dim() != 4:
        raise ValueError("E must be a tensor of shape (k, b, L, q)")
    q = E.shape[3]
    if not 1 <= q <= CLASS_MAX_STATES:
        raise ValueError("%s serves 1..%d states, got q = %d" % (name, CLASS_MAX_STATES, q))
    if state_class is None:
        raise ValueError("%s needs a class table (state_class)" % name)
    table, C = class_table(state_class, num_classes, q)
    if C > 16:
        raise ValueError("at most 16 classes, got %d" % C)
    return (ctypes.c_int * q)(*table), C


def class_posterior(A, pi, E, state_class, num_classes=None, eps=EPS, prob=True, log=False):
    """Class posteriors for up to 16 states by the chunked pipeline of posterior() (hmm_class_posterior)
    -> (prob (k,b,L,C) fp32 or None, log (k,b,L,C) fp32 or None, loglik (k,b) fp64): P_c[t] = the sum of the state
    posteriors of class c's states, with the bits posterior_decode's fused call compares; log = its log (-inf for a
    sum of 0).  Nothing of size (k,b,L,q) is written.  state_class: a sequence or an integer tensor of q classes, at
    most 16 of them.  Raises ValueError outside 1..16 states, without a table, above 16 classes, or with neither
    output asked for."""
    tab, C = _class_args("class_posterior", E, state_class, num_classes)
    if not (prob or log):
        raise ValueError("class_posterior: ask for prob, log or both")
    A, pi, E = _dev(A, "A"), _dev(pi, "pi"), _dev(E, "E")
    A, pi, dims = _shapes(A, E, pi)
    with torch.cuda.device(E.device):
        ws = _workspace(E.device, lib().hmm_class_posterior_workspace_bytes(*dims), CLASS_TAG)
        P = torch.empty(dims[:3] + (C,), dtype=torch.float32, device=E.device) if prob else None
        Lg = torch.empty(dims[:3] + (C,), dtype=torch.float32, device=E.device) if log else None
        ll = torch.empty(dims[:2], dtype=torch.float64, device=E.device)
        _check(lib().hmm_class_posterior(A.data_ptr(), pi.data_ptr(), E.data_ptr(), *dims, eps, tab, C,
                                         P.data_ptr() if prob else None, Lg.data_ptr() if log else None,
                                         ll.data_ptr(), ws.data_ptr(), ws.numel(), _stream(E.device)))
    return P, Lg, ll


def class_posterior_grad(A, pi, E, state_class, num_classes, grad_out, class_prob=None, mode=POST_LOG, eps=EPS):
    """Gradients of <grad_out, out> with out = the class posteriors (POST_PROB) or their logs (POST_LOG) of
    class_posterior -> (dA (k,q,q), dpi (k,q), dE (k,b,L,q)) by hmm_class_posterior_grad: grad_out is (k,b,L,C), read
    in place.  POST_PROB is posterior_grad(POST_PROB) with grad_out[..., state_class], bit for bit; POST_LOG needs
    class_prob, the forward's prob, and passes nothing through a class whose posterior is 0.  Raises ValueError
    outside 1..16 states, without a table, above 16 classes, and in log mode without class_prob."""
    tab, C = _class_args("class_posterior_grad", E, state_class, num_classes)
    if int(mode) not in (POST_PROB, POST_LOG):
        raise ValueError("class_posterior_grad supports mode POST_PROB or POST_LOG")
    if int(mode) == POST_LOG and class_prob is None:
        raise ValueError("class_posterior_grad: POST_LOG needs class_prob (class_posterior's prob)")
    A, pi, E, grad_out = _dev(A, "A"), _dev(pi, "pi"), _dev(E, "E"), _dev(grad_out, "grad_out")
    A, pi, dims = _shapes(A, E, pi)
    k, b, L, q = dims
    if tuple(grad_out.shape) != (k, b, L, C):
        raise ValueError("grad_out must have shape (k, b, L, C) = %s, got %s" % ((k, b, L, C), tuple(grad_out.shape)))
    if int(mode) == POST_LOG:
        class_prob = _dev(class_prob, "class_prob")
        if class_prob.shape != grad_out.shape:
            raise ValueError("class_prob must be shaped like grad_out")
    with torch.cuda.device(E.device):
        ws = _workspace(E.device, lib().hmm_class_posterior_grad_workspace_bytes(*dims, C), CLASS_GRAD_TAG)
        dA = torch.empty((k, q, q), dtype=torch.float32, device=E.device)
        dpi = torch.empty((k, q), dtype=torch.float32, device=E.device)
        dE = torch.empty_like(E)
        _check(lib().hmm_class_posterior_grad(
            A.data_ptr(), pi.data_ptr(), E.data_ptr(), *dims, eps, int(mode), tab, C,
            class_prob.data_ptr() if int(mode) == POST_LOG else None, grad_out.data_ptr(), dA.data_ptr(),
            dpi.data_ptr(), dE.data_ptr(), ws.data_ptr(), ws.numel(), _stream(E.device)))
    return dA, dpi, dE


def class_posterior_grad_serial_count(dims, device=None):
    """How many of the k*b sequences of the LAST class_posterior_grad call with shape `dims` on this device and stream
    were served by the whole-sequence sweeps (synchronises): the workspace begins with hmm_posterior_grad's layout."""
    return posterior_grad_serial_count(dims, device, _tag=CLASS_GRAD_TAG)
