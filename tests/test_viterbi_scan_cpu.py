"""Host side of hmm_viterbi_scan (no device needed): the new symbols, limits, the chunk length and workspace
queries, the routing predicate, and the argument checks in their stated order."""
import pytest

from hmm_layer_amd import build as hbuild
from hmm_layer_amd import engine

OK, BAD_SHAPE, Q_UNSUPPORTED, NULL_POINTER, WORKSPACE, BAD_ARGUMENT = 0, -1, -2, -3, -4, -6
SYMBOLS = ("hmm_viterbi_scan_max_states", "hmm_viterbi_scan_chunk_len", "hmm_viterbi_scan_pays",
           "hmm_viterbi_scan_workspace_bytes", "hmm_viterbi_scan")


@pytest.fixture(scope="module")
def lib():
    hbuild.build()
    return engine.lib()


def call(lib, k=1, b=2, L=300, q=29, ptrs=(256,) * 5, ws=256, nbytes=None):
    """hmm_viterbi_scan with placeholder device pointers: every call here returns before any HIP call."""
    logA, logpi, logE, path, score = ptrs
    if nbytes is None:
        nbytes = lib.hmm_viterbi_scan_workspace_bytes(k, b, L, q)
    return lib.hmm_viterbi_scan(logA, logpi, logE, k, b, L, q, path, score, ws, nbytes, None)


def test_symbols_and_limits(lib):
    for name in SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.hmm_viterbi_scan_max_states() == 64
    assert lib.hmm_viterbi_max_states() == 64
    assert lib.hmm_abi_version() == 3 == engine.ABI_VERSION
    assert lib.hmm_set_option(9, 0) == BAD_ARGUMENT          # no new option


def test_workspace_query(lib):
    assert lib.hmm_viterbi_scan_workspace_bytes(1, 1, 1, 1) > 0
    assert lib.hmm_viterbi_scan_workspace_bytes(2, 3, 1000, 64) > 0
    assert lib.hmm_viterbi_scan_workspace_bytes(2, 3, 1000, 64) % 256 == 0
    assert lib.hmm_viterbi_scan_workspace_bytes(1, 1, 1, 65) == 0
    assert lib.hmm_viterbi_scan_workspace_bytes(1, 0, 1, 29) == 0
    # 64-bit sizes: one backpointer byte per position and state, in 64-byte rows
    assert lib.hmm_viterbi_scan_workspace_bytes(1, 2, 17000000, 17) > 2 ** 31
    assert lib.hmm_viterbi_scan_workspace_bytes(1, 2, 17000000, 17) >= 2 * 17000000 * 64


def test_chunk_len(lib):
    for dims in ((1, 1, 1, 1), (1, 1, 100000, 29), (1, 1, 1000000, 43), (2, 1024, 100000, 57), (1, 5, 300, 64)):
        t = lib.hmm_viterbi_scan_chunk_len(*dims)
        assert t > 0 and t % 16 == 0 and t <= 512, (dims, t)
    assert lib.hmm_viterbi_scan_chunk_len(1, 1, 100, 65) == 0
    assert lib.hmm_viterbi_scan_chunk_len(1, 0, 100, 29) == 0
    with engine.option(engine.OPT_CHUNK, 48):
        assert lib.hmm_viterbi_scan_chunk_len(1, 1, 100000, 29) == 48
        assert lib.hmm_viterbi_scan_chunk_len(3, 7, 1000000, 64) == 48
    # a forced chunk length changes the number of operators, hence the workspace
    with engine.option(engine.OPT_CHUNK, 16):
        small = lib.hmm_viterbi_scan_workspace_bytes(1, 1, 100000, 29)
    with engine.option(engine.OPT_CHUNK, 512):
        large = lib.hmm_viterbi_scan_workspace_bytes(1, 1, 100000, 29)
    assert small > large


def test_error_codes_in_order(lib):
    none = (None,) * 5
    assert call(lib, q=65, ptrs=none, ws=None, nbytes=0) == Q_UNSUPPORTED      # q before pointers
    assert call(lib, b=0, ptrs=none, ws=None, nbytes=0) == BAD_SHAPE
    assert call(lib, b=0, q=65, ptrs=none, ws=None, nbytes=0) == BAD_SHAPE      # shape before q
    assert call(lib, k=0) == BAD_SHAPE and call(lib, L=0) == BAD_SHAPE and call(lib, q=0) == BAD_SHAPE
    assert call(lib, ptrs=none, ws=None, nbytes=0) == NULL_POINTER             # pointers before workspace
    for x in range(5):
        ptrs = [256] * 5
        ptrs[x] = None
        assert call(lib, ptrs=tuple(ptrs), nbytes=0) == NULL_POINTER
    assert call(lib, ws=None) == NULL_POINTER
    assert call(lib, nbytes=0) == WORKSPACE
    need = lib.hmm_viterbi_scan_workspace_bytes(1, 2, 300, 29)
    assert call(lib, nbytes=need - 1) == WORKSPACE
    assert call(lib, ws=256 + 8, nbytes=need + 256) == WORKSPACE               # misaligned


def test_pays_keeps_the_walk_where_it_fills_the_machine(lib):
    assert lib.hmm_viterbi_scan_pays(1, 1024, 100000, 29) == 0
    for q in (1, 15, 16, 65):                                  # outside 17..64 the question does not arise
        assert lib.hmm_viterbi_scan_pays(1, 1, 1000000, q) == 0
    assert lib.hmm_viterbi_scan_pays(1, 0, 100, 29) == 0


def test_python_entry_point_has_no_cpu_path(lib):
    import torch
    with pytest.raises(engine.EngineError):
        engine.viterbi_scan(torch.zeros(1, 29, 29), torch.zeros(1, 29), torch.zeros(1, 2, 3, 29))
