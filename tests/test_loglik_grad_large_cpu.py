"""Host side of hmm_loglik_grad_large (no device needed): limits, the option, argument checks in their order,
and a workspace that does not grow with the sequence length."""
import ctypes

import pytest

from hmm_layer_amd import build as hbuild
from hmm_layer_amd import engine

OK, BAD_SHAPE, Q_UNSUPPORTED, NULL_POINTER, WORKSPACE, BAD_ARGUMENT = 0, -1, -2, -3, -4, -6


@pytest.fixture(scope="module")
def lib():
    hbuild.build()
    return engine.lib()


def call(lib, k=1, b=2, L=3, q=70, ptrs=(256,) * 6, gw=None, ll=None, ws=256, nbytes=None):
    """hmm_loglik_grad_large with placeholder device pointers: every call here returns before any HIP call."""
    A, pi, E, dA, dpi, dE = ptrs
    if nbytes is None:
        nbytes = lib.hmm_loglik_grad_large_workspace_bytes(k, b, L, q)
    return lib.hmm_loglik_grad_large(A, pi, E, k, b, L, q, ctypes.c_float(1e-16), gw, dA, dpi, dE, ll, ws, nbytes, None)


def test_limits(lib):
    assert lib.hmm_loglik_grad_large_max_states() == 4096
    assert lib.hmm_grad_max_states() == 64
    assert lib.hmm_abi_version() == engine.ABI_VERSION


def test_option_round_trips(lib):
    assert engine.OPT_GLARGE == 8
    old = engine.set_option(engine.OPT_GLARGE, 2)
    try:
        assert engine.get_option(engine.OPT_GLARGE) == 2
        engine.set_option(engine.OPT_GLARGE, 1)
        assert engine.get_option(engine.OPT_GLARGE) == 1
    finally:
        engine.set_option(engine.OPT_GLARGE, old)
    assert engine.get_option(engine.OPT_GLARGE) == old
    with engine.option(engine.OPT_GLARGE, 2):
        assert engine.get_option(engine.OPT_GLARGE) == 2
    assert engine.get_option(engine.OPT_GLARGE) == old
    assert lib.hmm_set_option(9, 0) == BAD_ARGUMENT


def test_error_codes_in_order(lib):
    assert call(lib, k=0) == BAD_SHAPE
    assert call(lib, b=0, q=5000) == BAD_SHAPE                                 # shape before q
    assert call(lib, L=0) == BAD_SHAPE and call(lib, q=0) == BAD_SHAPE
    assert call(lib, q=4097, nbytes=0) == Q_UNSUPPORTED
    assert call(lib, q=4097, ptrs=(None,) * 6, ws=None, nbytes=0) == Q_UNSUPPORTED   # q before pointers
    for x in range(6):
        ptrs = [256] * 6
        ptrs[x] = None
        assert call(lib, ptrs=tuple(ptrs), nbytes=0) == NULL_POINTER          # pointers before workspace
    assert call(lib, ws=None) == NULL_POINTER
    need = lib.hmm_loglik_grad_large_workspace_bytes(1, 2, 3, 70)
    assert call(lib, nbytes=need - 1) == WORKSPACE
    assert call(lib, ws=256 + 8, nbytes=need + 256) == WORKSPACE              # misaligned
    # forcing the walk above its limit is refused, not switched
    with engine.option(engine.OPT_GLARGE, 1):
        assert call(lib, q=129) == BAD_ARGUMENT
        assert call(lib, q=1027) == BAD_ARGUMENT
        assert call(lib, q=129, nbytes=0) == WORKSPACE                        # after the workspace check


def test_workspace_query(lib):
    assert lib.hmm_loglik_grad_large_workspace_bytes(1, 1, 1, 4097) == 0
    assert lib.hmm_loglik_grad_large_workspace_bytes(0, 1, 1, 65) == 0
    for q in (1, 65, 128, 129, 1027, 4096):
        assert lib.hmm_loglik_grad_large_workspace_bytes(2, 1024, 10, q) > 0
    for q in (65, 71, 128, 129, 1027):
        short = lib.hmm_loglik_grad_large_workspace_bytes(2, 1024, 10, q)
        assert short == lib.hmm_loglik_grad_large_workspace_bytes(2, 1024, 100000, q)
        assert short % 256 == 0
    # the walk keeps one q x q partial per sequence; the GEMMs need O(b q) and k q^2 only
    walk = lib.hmm_loglik_grad_large_workspace_bytes(1, 1024, 10, 128)
    assert walk >= 1024 * 128 * 128 * 4
    gemm = lib.hmm_loglik_grad_large_workspace_bytes(1, 1024, 10, 129)
    assert gemm < 16 * 1024 * 129 * 4 + 129 * 129 * 8 + (1 << 20)


def test_python_entry_point_has_no_cpu_path(lib):
    import torch
    with pytest.raises(engine.EngineError):
        engine.loglik_grad_large(torch.eye(70)[None], torch.ones(1, 70) / 70, torch.rand(1, 2, 3, 70))
