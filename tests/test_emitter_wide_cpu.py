"""Host side of hmm_gene_emissions_wide / hmm_gene_emissions_grad_wide (no device needed): the exported symbols,
the limits, argument checks in their order, the workspace query, the untouched limits of the 64-state entry points,
the module and the oracle against the reference's recorded outputs for 43, 71 and 253 states
(tests/golden/emitter_wide.npz), and the routing rule."""
import ctypes

import pytest
import torch

from hmm_layer_amd import build as hbuild
from hmm_layer_amd import engine
from hmm_layer_amd.gene_pred_hmm_emitter import GenePredHMMEmitter
from oracle import params

OK, BAD_SHAPE, Q_UNSUPPORTED, NULL_POINTER, WORKSPACE = 0, -1, -2, -3, -4
CODONS = dict(start_codons=[("ATG", 1.)], stop_codons=[("TAG", .34), ("TAA", .33), ("TGA", .33)],
              intron_begin_pattern=[("NGT", .99), ("NGC", .005), ("NAT", .005)],
              intron_end_pattern=[("AGN", .99), ("ACN", .01)])
F = ctypes.c_float
MIB16 = 16 << 20


@pytest.fixture(scope="module")
def lib():
    hbuild.build()
    return engine.lib()


def fwd(lib, name="hmm_gene_emissions_wide", b=2, L=3, s=15, rows=43, nc=9, q=43, ptrs=(256,) * 6):
    """The forward with placeholder device pointers: every call here returns before any HIP call."""
    x, B, state_row, codon, state_codon, E = ptrs
    return getattr(lib, name)(x, b, L, s, B, rows, state_row, codon, nc, state_codon, q, F(1.0 / 4096), F(0.0), 1, E, None)


def grad(lib, name="hmm_gene_emissions_grad_wide", b=2, L=3, s=15, rows=43, nc=9, q=43, ptrs=(256,) * 8, ws=256,
         nbytes=None):
    x, B, state_row, codon, state_codon, dE, dx, dB = ptrs
    if nbytes is None:
        nbytes = getattr(lib, name + "_workspace_bytes")(b, L, s, rows, q)
    return getattr(lib, name)(x, b, L, s, B, rows, state_row, codon, nc, state_codon, q, F(1.0 / 4096), F(1e-7), 1,
                              dE, dx, dB, ws, nbytes, None)


def test_symbols_abi_and_limits(lib):
    for name in ("hmm_gene_emissions_wide_max_states", "hmm_gene_emissions_wide",
                 "hmm_gene_emissions_grad_wide_workspace_bytes", "hmm_gene_emissions_grad_wide"):
        assert hasattr(lib, name) and name in engine._SIGNATURES
    assert lib.hmm_abi_version() == 3 == engine.ABI_VERSION
    assert lib.hmm_gene_emissions_wide_max_states() == 256
    for kw in (dict(q=257), dict(rows=257), dict(s=33), dict(nc=17)):
        assert fwd(lib, **kw) == Q_UNSUPPORTED, kw
        assert grad(lib, nbytes=0, **kw) == Q_UNSUPPORTED, kw


def test_error_codes_in_order(lib):
    for call in (fwd, lambda lib, **kw: grad(lib, nbytes=0, **kw)):
        for kw in (dict(b=0), dict(L=0), dict(s=0), dict(rows=0), dict(q=0), dict(nc=-1)):
            assert call(lib, **kw) == BAD_SHAPE, kw
        assert call(lib, b=0, q=257) == BAD_SHAPE                                  # shape before limits
    assert fwd(lib, q=257, ptrs=(None,) * 6) == Q_UNSUPPORTED                      # limits before pointers
    assert grad(lib, q=257, ptrs=(None,) * 8, ws=None, nbytes=0) == Q_UNSUPPORTED
    for i in range(6):
        ptrs = [256] * 6
        ptrs[i] = None
        assert fwd(lib, ptrs=tuple(ptrs)) == NULL_POINTER, i
        ptrs = [256] * 8
        ptrs[i] = None
        assert grad(lib, ptrs=tuple(ptrs), nbytes=0) == NULL_POINTER, i            # pointers before workspace
    assert grad(lib, ptrs=(256,) * 6 + (None, None), nbytes=0) == NULL_POINTER     # both outputs NULL
    assert grad(lib, ws=None) == NULL_POINTER
    no_codon = (256, 256, 256, None, 256, 256, 256, 256)
    assert grad(lib, nc=0, ptrs=no_codon, nbytes=0) == WORKSPACE                   # no tables: codon may be NULL
    need = lib.hmm_gene_emissions_grad_wide_workspace_bytes(2, 3, 15, 43, 43)
    for ptrs in ((256,) * 8, (256,) * 6 + (None, 256), (256,) * 6 + (256, None)):
        assert grad(lib, ptrs=ptrs, nbytes=need - 1) == WORKSPACE                  # one byte short
        assert grad(lib, ptrs=ptrs, ws=256 + 128, nbytes=need + 256) == WORKSPACE  # misaligned


def test_workspace_query(lib):
    wsb = lib.hmm_gene_emissions_grad_wide_workspace_bytes
    for args in ((2, 3, 15, 43, 257), (2, 3, 15, 257, 43), (2, 3, 33, 43, 43), (0, 3, 15, 43, 43), (2, 0, 15, 43, 43),
                 (2, 3, 0, 43, 43), (2, 3, 15, 0, 43), (2, 3, 15, 43, 0)):
        assert wsb(*args) == 0, args
    for s, rows, q in ((15, 37, 43), (15, 57, 57), (15, 61, 71), (15, 253, 253), (32, 256, 256), (1, 1, 1), (7, 256, 64)):
        n = wsb(1000, 1000, s, rows, q)                                            # b L = 1e6
        assert n > 0 and n % 256 == 0
        assert n == wsb(10000, 10000, s, rows, q)                                  # b L = 1e8
        assert n <= MIB16 + 256
        # one (rows, s) partial per workgroup, at most 1024 workgroups
        assert n <= (1024 * rows * s * 4 + 255) // 256 * 256
        assert n >= rows * s * 4
    assert wsb(1000, 1000, 32, 256, 256) == MIB16                                  # 512 partials of 32 KiB


def test_the_64_state_entry_points_keep_their_limits(lib):
    assert fwd(lib, "hmm_gene_emissions", q=64, rows=32, ptrs=(None,) * 6) == NULL_POINTER
    assert fwd(lib, "hmm_gene_emissions", q=65, rows=32) == Q_UNSUPPORTED
    assert fwd(lib, "hmm_gene_emissions", q=64, rows=33) == Q_UNSUPPORTED
    assert grad(lib, "hmm_gene_emissions_grad", q=65, rows=32, nbytes=0) == Q_UNSUPPORTED
    assert grad(lib, "hmm_gene_emissions_grad", q=64, rows=33, nbytes=0) == Q_UNSUPPORTED
    assert lib.hmm_gene_emissions_grad_workspace_bytes(2, 3, 15, 32, 65) == 0
    assert lib.hmm_gene_emissions_grad_workspace_bytes(2, 3, 15, 33, 64) == 0


def test_python_entry_points_have_no_cpu_path(lib):
    x = torch.rand(2, 3, 20)
    B = torch.softmax(torch.rand(43, 15), -1)
    row = torch.arange(43, dtype=torch.int32)
    cod = torch.full((43,), -1, dtype=torch.int32)
    with pytest.raises(engine.EngineError):
        engine.gene_emissions_wide(x, B, row, torch.rand(2, 9, 64), cod)
    with pytest.raises(engine.EngineError):
        engine.gene_emissions_grad_wide(x, B, row, torch.rand(2, 9, 64), cod, torch.rand(2, 3, 43))


def test_module_and_oracle_equal_the_reference(golden):
    """The torch-op module (n_mass_compat=True: the reference mutates its input) and the oracle's restatement are
    bit-identical to the reference's forward for 43, 71 and 253 states, training off and on.  The inference outputs
    hold exact zeros, so the comparison is absolute: torch.equal."""
    z = golden("emitter_wide")
    x = torch.from_numpy(z["x"])
    assert tuple(x.shape) == (1, 2, 24, 20)
    tab = params.codon_table(**params.DEFAULT_CODONS)
    assert [tuple(m) for m in z["models"]] == [(3, 1), (5, 1), (18, 0)]
    for c, shared in z["models"]:
        c, shared = int(c), bool(shared)
        tag = "c%d_%s" % (c, "shared" if shared else "unshared")
        kernel = torch.from_numpy(z[tag + "_kernel"])
        em = GenePredHMMEmitter(**CODONS, num_copies=c, share_intron_parameters=shared, n_mass_compat=True)
        em.build((1, 2, 24, 15))
        assert em.num_states == 1 + 14 * c and tuple(kernel.shape) == (1, em.kernel_rows(), 15)
        with torch.no_grad():
            em.emission_kernel.copy_(kernel)
        em.recurrent_init()
        for training in (False, True):
            want = torch.from_numpy(z[tag + ("_E_training" if training else "_E")])
            assert tuple(want.shape) == (1, 2, 24, em.num_states)
            if not training:
                assert bool((want == 0).any())
            with torch.no_grad():
                assert torch.equal(em(x.clone(), training=training), want), (tag, training)
            got = params.gene_emissions(x, kernel, tab, copies=c, share_intron=shared, training=training, d5_compat=True)
            assert torch.equal(got, want), (tag, training)


def emitter(copies, shared=True, **kw):
    em = GenePredHMMEmitter(**CODONS, num_copies=copies, share_intron_parameters=shared, **kw)
    em.build((1, 2, 24, 15))
    return em


def test_routing_rule(lib):
    """Which kernels serve which model: a plain function of (states, rows, embeddings)."""
    route = engine.gene_emissions_routes_wide
    assert route(64, 32) is False and route(15, 15) is False and route(1, 1) is False
    assert route(65, 32) is True and route(64, 33) is True and route(256, 256) is True and route(43, 37) is True
    assert route(257, 32) is None and route(64, 257) is None
    assert emitter(1).fused_route() == "gene" and emitter(2).fused_route() == "gene"              # 15, 29 states
    assert emitter(2, False).fused_route() == "gene"                                             # 29 rows
    assert emitter(3).fused_route() == "wide"                                                    # 43 states, 37 rows
    assert emitter(3, False).fused_route() == "wide" and emitter(4, False).fused_route() == "wide"
    assert emitter(5).fused_route() == "wide" and emitter(18, False).fused_route() == "wide"     # 71, 253 states
    assert emitter(19).fused_route() is None                                                     # 267 states
    # the embedding kernels stop at 64 states and 32 rows
    emb = dict(emit_embeddings=True, embedding_dim=4)
    assert emitter(2, **emb).fused_route() == "gene"
    assert emitter(3, **emb).fused_route() is None and emitter(5, **emb).fused_route() is None
    # can_fuse: never on CPU tensors
    x = torch.zeros(1, 2, 24, 20)
    for em in (emitter(1), emitter(3), emitter(5), emitter(19)):
        assert em.can_fuse(x) is False
