"""Host side of hmm_loglik_grad_scan (no device needed): the new symbols, limits, the chunk length and workspace
queries, the routing predicate, and the argument checks in their stated order."""
import pytest

from hmm_layer_amd import build as hbuild
from hmm_layer_amd import engine

OK, BAD_SHAPE, Q_UNSUPPORTED, NULL_POINTER, WORKSPACE, BAD_ARGUMENT = 0, -1, -2, -3, -4, -6
SYMBOLS = ("hmm_loglik_grad_scan_max_states", "hmm_loglik_grad_scan_chunk_len", "hmm_loglik_grad_scan_pays",
           "hmm_loglik_grad_scan_workspace_bytes", "hmm_loglik_grad_scan_serial_count", "hmm_loglik_grad_scan")
PTRS = ("A", "pi", "E", "dA", "dpi", "dE")


@pytest.fixture(scope="module")
def lib():
    hbuild.build()
    return engine.lib()


def call(lib, k=1, b=2, L=300, q=43, ptrs=(256,) * 6, gw=None, ll=None, ws=256, nbytes=None):
    """hmm_loglik_grad_scan with placeholder device pointers: every call here returns before any HIP call."""
    A, pi, E, dA, dpi, dE = ptrs
    if nbytes is None:
        nbytes = lib.hmm_loglik_grad_scan_workspace_bytes(k, b, L, q)
    return lib.hmm_loglik_grad_scan(A, pi, E, k, b, L, q, 1e-16, gw, dA, dpi, dE, ll, ws, nbytes, None)


def test_symbols_and_limits(lib):
    for name in SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.hmm_loglik_grad_scan_max_states() == 64
    assert lib.hmm_grad_max_states() == 64
    assert lib.hmm_abi_version() == 3 == engine.ABI_VERSION
    assert lib.hmm_set_option(9, 0) == BAD_ARGUMENT          # no new option


def test_workspace_query(lib):
    for dims in ((2, 3, 1000, 64), (1, 1, 1, 17)):
        n = lib.hmm_loglik_grad_scan_workspace_bytes(*dims)
        assert n > 0 and n % 256 == 0, dims
        k, b, L, q = dims
        assert n >= 2 * k * b * L * q * 4, dims                 # the two value arrays
    assert lib.hmm_loglik_grad_scan_workspace_bytes(1, 1, 1, 65) == 0
    assert lib.hmm_loglik_grad_scan_workspace_bytes(1, 0, 1, 29) == 0
    # 64-bit sizes
    big = (1, 64, 1000000, 64)
    assert lib.hmm_loglik_grad_scan_workspace_bytes(*big) >= 2 * 64 * 1000000 * 64 * 4 > 2 ** 32
    # q <= 16: hmm_loglik_grad's own plan
    assert lib.hmm_loglik_grad_scan_workspace_bytes(2, 3, 1000, 15) == lib.hmm_loglik_grad_workspace_bytes(2, 3, 1000, 15)
    # a forced chunk length changes the number of chunk operators, hence the workspace
    with engine.option(engine.OPT_CHUNK, 16):
        small = lib.hmm_loglik_grad_scan_workspace_bytes(1, 1, 100000, 43)
    with engine.option(engine.OPT_CHUNK, 512):
        large = lib.hmm_loglik_grad_scan_workspace_bytes(1, 1, 100000, 43)
    assert small > large


def test_32_bit_row_offsets_make_a_shape_unsupported(lib):
    """L * q * 4 >= 2^31: refused by every query and by the call, never silently wrong."""
    dims = (1, 1, 9000000, 64)
    assert 9000000 * 64 * 4 >= 2 ** 31
    assert lib.hmm_loglik_grad_scan_workspace_bytes(*dims) == 0
    assert lib.hmm_loglik_grad_scan_chunk_len(*dims) == 0
    assert lib.hmm_loglik_grad_scan_pays(*dims) == 0
    assert call(lib, 1, 1, 9000000, 64, nbytes=1 << 40) == BAD_SHAPE
    assert lib.hmm_loglik_grad_scan_workspace_bytes(1, 1, 8000000, 64) > 0


def test_chunk_len(lib):
    for dims in ((1, 1, 1, 1), (1, 1, 100000, 29), (1, 1, 1000000, 43), (2, 1024, 100000, 57), (1, 5, 300, 64),
                 (1, 32, 9999, 24), (1, 3, 100, 17)):
        t = lib.hmm_loglik_grad_scan_chunk_len(*dims)
        assert t > 0 and t % 16 == 0 and t <= 512, (dims, t)
    assert lib.hmm_loglik_grad_scan_chunk_len(1, 1, 100, 65) == 0
    assert lib.hmm_loglik_grad_scan_chunk_len(1, 0, 100, 29) == 0
    with engine.option(engine.OPT_CHUNK, 48):
        assert lib.hmm_loglik_grad_scan_chunk_len(1, 1, 100000, 24) == 48
        assert lib.hmm_loglik_grad_scan_chunk_len(3, 7, 1000000, 64) == 48


def test_pays_is_zero_where_the_question_does_not_arise(lib):
    for q in (1, 15, 16, 65, 100):
        assert lib.hmm_loglik_grad_scan_pays(1, 1, 1000000, q) == 0
    assert lib.hmm_loglik_grad_scan_pays(1, 0, 100, 43) == 0
    for q in (17, 24, 43, 57, 64):                             # below 4 chunks
        T = lib.hmm_loglik_grad_scan_chunk_len(1, 4, 9999, q)
        assert lib.hmm_loglik_grad_scan_pays(1, 4, 3 * T, q) == 0
        assert lib.hmm_loglik_grad_scan_pays(1, 4, 1, q) == 0
    assert lib.hmm_loglik_grad_scan_pays(1, 32, 9999, 29) == 0   # hmm_loglik_grad already runs this per chunk
    with engine.option(engine.OPT_PGCHUNK, 0):                 # the whole-sequence sweeps are asked for
        for dims in ((1, 1, 100000, 43), (1, 4, 100000, 24), (1, 32, 9999, 64)):
            assert lib.hmm_loglik_grad_scan_pays(*dims) == 0


def test_error_codes_in_order(lib):
    none = (None,) * 6
    assert call(lib, q=65, ptrs=none, ws=None, nbytes=0) == Q_UNSUPPORTED      # q before pointers
    assert call(lib, b=0, ptrs=none, ws=None, nbytes=0) == BAD_SHAPE
    assert call(lib, b=0, q=65, ptrs=none, ws=None, nbytes=0) == BAD_SHAPE      # shape before q
    assert call(lib, k=0) == BAD_SHAPE and call(lib, L=0) == BAD_SHAPE and call(lib, q=0) == BAD_SHAPE
    for q in (15, 24, 43):
        assert call(lib, q=q, ptrs=none, ws=None, nbytes=0) == NULL_POINTER    # pointers before workspace
        for x in range(6):
            ptrs = [256] * 6
            ptrs[x] = None
            assert call(lib, q=q, ptrs=tuple(ptrs), nbytes=0) == NULL_POINTER, PTRS[x]
        assert call(lib, q=q, ws=None) == NULL_POINTER
        assert call(lib, q=q, nbytes=0) == WORKSPACE
        need = lib.hmm_loglik_grad_scan_workspace_bytes(1, 2, 300, q)
        assert call(lib, q=q, nbytes=need - 1) == WORKSPACE
        assert call(lib, q=q, ws=256 + 8, nbytes=need + 256) == WORKSPACE      # misaligned
    assert lib.hmm_loglik_grad_scan_serial_count(1, 0, 300, 43, None, 0) == BAD_SHAPE
    assert lib.hmm_loglik_grad_scan_serial_count(1, 2, 300, 65, None, 0) == Q_UNSUPPORTED
    assert lib.hmm_loglik_grad_scan_serial_count(1, 2, 300, 43, None, 0) == NULL_POINTER
    assert lib.hmm_loglik_grad_scan_serial_count(1, 2, 300, 43, 256, 0) == WORKSPACE


def test_python_entry_point_has_no_cpu_path(lib):
    import torch
    with pytest.raises(engine.EngineError):
        engine.loglik_grad_scan(torch.zeros(1, 43, 43), torch.zeros(1, 43), torch.zeros(1, 2, 3, 43))
