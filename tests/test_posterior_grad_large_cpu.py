"""Host side of hmm_posterior_grad_large (no device needed): limits, argument checks in their order, the
workspace query and its budget, and the Python entry point's refusals."""
import ctypes

import pytest

from hmm_layer_amd import build as hbuild
from hmm_layer_amd import engine

OK, BAD_SHAPE, Q_UNSUPPORTED, NULL_POINTER, WORKSPACE, BAD_ARGUMENT = 0, -1, -2, -3, -4, -6


@pytest.fixture(scope="module")
def lib():
    hbuild.build()
    return engine.lib()


def call(lib, k=1, b=2, L=3, q=70, mode=engine.POST_LOG, ptrs=(256,) * 7, ws=256, nbytes=None):
    """hmm_posterior_grad_large with placeholder device pointers: every call here returns before any HIP call."""
    A, pi, E, G, dA, dpi, dE = ptrs
    if nbytes is None:
        nbytes = lib.hmm_posterior_grad_large_workspace_bytes(k, b, L, q)
    return lib.hmm_posterior_grad_large(A, pi, E, k, b, L, q, ctypes.c_float(1e-16), mode, G, dA, dpi, dE, ws, nbytes,
                                        None)


def test_limits(lib):
    assert lib.hmm_posterior_grad_large_max_states() == 4096
    assert lib.hmm_posterior_grad_max_states() == 64
    assert lib.hmm_abi_version() == engine.ABI_VERSION
    assert lib.hmm_set_option(9, 0) == BAD_ARGUMENT                          # no new option: HMM_OPT_GLARGE serves


def test_error_codes_in_order(lib):
    assert call(lib, k=0) == BAD_SHAPE
    assert call(lib, b=0, q=5000, mode=7) == BAD_SHAPE                        # shape before q and mode
    assert call(lib, L=0) == BAD_SHAPE and call(lib, q=0) == BAD_SHAPE
    assert call(lib, q=4097, mode=7, nbytes=0) == Q_UNSUPPORTED              # q before mode
    assert call(lib, q=4097, ptrs=(None,) * 7, ws=None, nbytes=0) == Q_UNSUPPORTED
    for mode in (-1, engine.POST_LOG_NO_LL, 3):
        assert call(lib, mode=mode, ptrs=(None,) * 7, ws=None, nbytes=0) == BAD_ARGUMENT   # mode before pointers
    assert call(lib, mode=engine.POST_PROB, nbytes=0) == WORKSPACE
    for x in range(7):
        ptrs = [256] * 7
        ptrs[x] = None
        assert call(lib, ptrs=tuple(ptrs), nbytes=0) == NULL_POINTER          # pointers before workspace
    assert call(lib, ws=None) == NULL_POINTER
    need = lib.hmm_posterior_grad_large_workspace_bytes(1, 2, 3, 70)
    assert call(lib, nbytes=need - 1) == WORKSPACE
    assert call(lib, ws=256 + 8, nbytes=need + 256) == WORKSPACE              # misaligned
    # forcing the walk above its limit is refused, not switched
    with engine.option(engine.OPT_GLARGE, 1):
        assert call(lib, q=129) == BAD_ARGUMENT
        assert call(lib, q=1027) == BAD_ARGUMENT
        assert call(lib, q=129, nbytes=0) == WORKSPACE                        # after the workspace check


def test_workspace_query(lib):
    assert lib.hmm_posterior_grad_large_workspace_bytes(1, 1, 1, 4097) == 0
    for dims in ((0, 1, 1, 65), (1, 0, 1, 65), (1, 1, 0, 65), (1, 1, 1, 0)):
        assert lib.hmm_posterior_grad_large_workspace_bytes(*dims) == 0
    for q in (1, 65, 128, 129, 1027, 4096):
        n = lib.hmm_posterior_grad_large_workspace_bytes(2, 1024, 10, q)
        assert n > 0 and n % 256 == 0


@pytest.mark.parametrize("k,b,q", [(1, 1024, 71), (2, 300, 128), (1, 1024, 129), (2, 64, 1027), (1, 3, 4096)])
def test_workspace_grows_with_L_within_its_budget(lib, k, b, q):
    """Both value recursions are kept at every position: per position at most the three k*b*q float arrays and the
    k*b normalisers; what does not depend on L is per-sequence q x q partials (walk) or O(k b q) + k q^2 doubles."""
    per_pos = 3 * k * b * q * 4 + k * b * 4
    sizes = {L: lib.hmm_posterior_grad_large_workspace_bytes(k, b, L, q) for L in (1, 10, 1000)}
    assert sizes[1] < sizes[10] < sizes[1000]
    for L0, L1 in ((1, 10), (10, 1000)):
        assert sizes[L1] - sizes[L0] <= per_pos * (L1 - L0) + 8 * 256
    fixed = sizes[1] - per_pos
    walk = 2 * k * b * q * q * 4 if q <= 128 else 0
    assert fixed <= walk + 16 * k * b * q * 4 + k * q * q * 12 + 4 * k * b * 64 * 4 + (1 << 20)


def test_python_entry_point(lib):
    import torch
    A, pi, E = torch.eye(70)[None], torch.ones(1, 70) / 70, torch.rand(1, 2, 3, 70)
    with pytest.raises(ValueError):
        engine.posterior_grad_large(A, pi, E, torch.ones_like(E), mode=engine.POST_LOG_NO_LL)
    with pytest.raises(engine.EngineError):                                   # no CPU path
        engine.posterior_grad_large(A, pi, E, torch.ones_like(E))
    with pytest.raises(engine.EngineError):
        engine.posterior_grad_large(A, pi, E, torch.ones_like(E), mode=engine.POST_PROB)
