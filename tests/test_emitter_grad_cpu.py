"""Host side of hmm_gene_emissions_grad (no device needed): the exported symbols, the workspace query, argument
checks in their order, the Python entry point's refusal of CPU tensors, and the emitter's fused_training switch."""
import ctypes

import pytest

from hmm_layer_amd import build as hbuild
from hmm_layer_amd import engine

OK, BAD_SHAPE, Q_UNSUPPORTED, NULL_POINTER, WORKSPACE = 0, -1, -2, -3, -4
CODONS = dict(start_codons=[("ATG", 1.)], stop_codons=[("TAG", .34), ("TAA", .33), ("TGA", .33)],
              intron_begin_pattern=[("NGT", .99), ("NGC", .005), ("NAT", .005)],
              intron_end_pattern=[("AGN", .99), ("ACN", .01)])
# x, B, state_row, codon, state_codon, dE, dx, dB
NAMES = ("x", "B", "state_row", "codon", "state_codon", "dE", "dx", "dB")


@pytest.fixture(scope="module")
def lib():
    hbuild.build()
    return engine.lib()


def call(lib, b=2, L=3, s=15, rows=15, nc=9, q=15, ptrs=(256,) * 8, ws=256, nbytes=None):
    """hmm_gene_emissions_grad with placeholder device pointers: every call here returns before any HIP call."""
    x, B, state_row, codon, state_codon, dE, dx, dB = ptrs
    if nbytes is None:
        nbytes = lib.hmm_gene_emissions_grad_workspace_bytes(b, L, s, rows, q)
    return lib.hmm_gene_emissions_grad(x, b, L, s, B, rows, state_row, codon, nc, state_codon, q,
                                       ctypes.c_float(1.0 / 4096), ctypes.c_float(1e-7), 1, dE, dx, dB, ws, nbytes, None)


def test_symbols_and_abi(lib):
    assert hasattr(lib, "hmm_gene_emissions_grad") and hasattr(lib, "hmm_gene_emissions_grad_workspace_bytes")
    assert lib.hmm_abi_version() == 3 == engine.ABI_VERSION


def test_workspace_query(lib):
    wsb = lib.hmm_gene_emissions_grad_workspace_bytes
    for b, L, s, rows, q in ((1, 1, 1, 1, 1), (3, 5, 15, 15, 15), (2, 1100, 7, 15, 15), (5, 4099, 20, 25, 29),
                             (64, 9999, 32, 32, 64)):
        n = wsb(b, L, s, rows, q)
        assert n > 0 and n % 256 == 0
    assert wsb(2, 3, 15, 15, 65) == 0
    assert wsb(2, 3, 33, 15, 15) == 0
    assert wsb(2, 3, 15, 33, 15) == 0
    assert wsb(0, 3, 15, 15, 15) == 0
    # one (rows, s) partial per workgroup; the grid stops growing at 1024 workgroups of 8 runs of 1024 positions
    full = wsb(1024, 8 * 1024, 15, 15, 15)
    assert full == 1024 * 15 * 15 * 4
    assert wsb(1024, 100000, 15, 15, 15) == full and wsb(4096, 100000, 15, 15, 15) == full
    assert wsb(1, 1024, 15, 15, 15) < wsb(1, 100 * 8 * 1024, 15, 15, 15) < full


def test_error_codes_in_order(lib):
    assert call(lib, b=0) == BAD_SHAPE and call(lib, L=0) == BAD_SHAPE and call(lib, s=0) == BAD_SHAPE
    assert call(lib, rows=0) == BAD_SHAPE and call(lib, q=0) == BAD_SHAPE and call(lib, nc=-1) == BAD_SHAPE
    assert call(lib, b=0, q=65, nbytes=0) == BAD_SHAPE                         # shape before limits
    for kw in (dict(q=65), dict(s=33), dict(rows=33), dict(nc=17)):
        assert call(lib, nbytes=0, **kw) == Q_UNSUPPORTED
        assert call(lib, ptrs=(None,) * 8, ws=None, nbytes=0, **kw) == Q_UNSUPPORTED    # limits before pointers
    for i, name in enumerate(NAMES[:6]):
        ptrs = [256] * 8
        ptrs[i] = None
        assert call(lib, ptrs=tuple(ptrs), nbytes=0) == NULL_POINTER, name    # pointers before workspace
    assert call(lib, ptrs=(256,) * 6 + (None, None), nbytes=0) == NULL_POINTER  # both outputs NULL
    assert call(lib, ws=None) == NULL_POINTER
    no_codon = (256, 256, 256, None, 256, 256, 256, 256)
    assert call(lib, nc=0, ptrs=no_codon, nbytes=0) == WORKSPACE               # no tables: codon may be NULL
    need = lib.hmm_gene_emissions_grad_workspace_bytes(2, 3, 15, 15, 15)
    for ptrs in ((256,) * 8, (256,) * 6 + (None, 256), (256,) * 6 + (256, None)):
        assert call(lib, ptrs=ptrs, nbytes=need - 1) == WORKSPACE
        assert call(lib, ptrs=ptrs, ws=256 + 8, nbytes=need + 256) == WORKSPACE        # misaligned


def test_python_entry_point_has_no_cpu_path(lib):
    import torch
    x = torch.rand(2, 3, 20)
    B = torch.softmax(torch.rand(15, 15), -1)
    row = torch.arange(15, dtype=torch.int32)
    cod = torch.full((15,), -1, dtype=torch.int32)
    with pytest.raises(engine.EngineError):
        engine.gene_emissions_grad(x, B, row, torch.rand(2, 9, 64), cod, torch.rand(2, 3, 15))


def test_fused_training_round_trips_through_config():
    from hmm_layer_amd.gene_pred_hmm_emitter import GenePredHMMEmitter
    assert GenePredHMMEmitter(**CODONS).fused_training is False
    assert GenePredHMMEmitter(**CODONS).get_config()["fused_training"] is False
    em = GenePredHMMEmitter(**CODONS, fused_training=True, num_copies=2)
    cfg = em.get_config()
    assert cfg["fused_training"] is True
    twin = GenePredHMMEmitter.from_config(cfg)
    assert twin.fused_training is True and twin.num_copies == 2 and twin.get_config() == cfg
    assert hasattr(twin, "forward_fused_trainable")
