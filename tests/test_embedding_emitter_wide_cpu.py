"""Host side of hmm_embedding_emissions_wide / hmm_embedding_emissions_grad_wide (no device needed): the exported
symbols, the limits, the argument checks in their stated order, the workspace query, the untouched limits of the
64-state pair, the routing rules of the engine and of the emitter module, and the row-block formulation of the
backward in fp64 torch against autograd."""
import pytest
import torch

from hmm_layer_amd import build as hbuild
from hmm_layer_amd import engine
from hmm_layer_amd.gene_pred_hmm_emitter import GenePredHMMEmitter

OK, BAD_SHAPE, Q_UNSUPPORTED, NULL_POINTER, WORKSPACE, BAD_ARGUMENT = 0, -1, -2, -3, -4, -6
CODONS = dict(start_codons=[("ATG", 1.)], stop_codons=[("TAG", .34), ("TAA", .33), ("TGA", .33)],
              intron_begin_pattern=[("NGT", .99), ("NGC", .005), ("NAT", .005)],
              intron_end_pattern=[("AGN", .99), ("ACN", .01)])
FWD_INPUTS = ("emb", "mean", "inv_std", "log_norm", "state_row", "E")
GRAD_INPUTS = ("emb", "mean", "inv_std", "log_norm", "state_row", "dE")
MIB16 = 16 << 20


@pytest.fixture(scope="module")
def lib():
    hbuild.build()
    return engine.lib()


def fwd(lib, name="hmm_embedding_emissions_wide", b=2, L=300, d=20, rows=37, q=43, ld=None, multiply=1, **inputs):
    """The forward with placeholder device pointers: every call here returns before any HIP call."""
    p = {n: inputs.get(n, 256) for n in FWD_INPUTS}
    return getattr(lib, name)(p["emb"], d + 20 if ld is None else ld, b, L, d, p["mean"], p["inv_std"], p["log_norm"],
                              rows, p["state_row"], q, 1.0, 0.0, multiply, p["E"], None)


def grad(lib, name="hmm_embedding_emissions_grad_wide", b=2, L=300, d=20, rows=37, q=43, ld=None, ldd=None, E_in=256,
         dE_in=256, demb=256, tabs=(256, 256, 256), ws=256, nbytes=None, **inputs):
    p = {n: inputs.get(n, 256) for n in GRAD_INPUTS}
    if nbytes is None:
        nbytes = getattr(lib, name + "_workspace_bytes")(b, L, d, rows, q)
    return getattr(lib, name)(p["emb"], d + 20 if ld is None else ld, b, L, d, p["mean"], p["inv_std"], p["log_norm"],
                              rows, p["state_row"], q, 1.0, 0.0, E_in, p["dE"], dE_in, demb, d if ldd is None else ldd,
                              *tabs, ws, nbytes, None)


def test_symbols_abi_and_limits(lib):
    for name in ("hmm_embedding_emissions_wide_max_states", "hmm_embedding_emissions_wide",
                 "hmm_embedding_emissions_grad_wide_workspace_bytes", "hmm_embedding_emissions_grad_wide"):
        assert hasattr(lib, name) and name in engine._SIGNATURES, name
    assert lib.hmm_abi_version() == 3 == engine.ABI_VERSION
    assert lib.hmm_embedding_emissions_wide_max_states() == 256
    dmax = lib.hmm_embedding_emissions_max_dim()
    assert dmax == 4096 == lib.hmm_embedding_emissions_grad_max_dim()
    # the limits pass at the corner: the next check (pointers) answers
    none_f, none_g = {n: None for n in FWD_INPUTS}, {n: None for n in GRAD_INPUTS}
    assert fwd(lib, q=256, rows=256, d=dmax, **none_f) == NULL_POINTER
    assert grad(lib, q=256, rows=256, d=dmax, ws=None, nbytes=0, **none_g) == NULL_POINTER
    for kw in (dict(q=257), dict(rows=257), dict(d=dmax + 1)):
        assert fwd(lib, **kw) == Q_UNSUPPORTED, kw
        assert grad(lib, nbytes=0, **kw) == Q_UNSUPPORTED, kw


def test_forward_error_codes_in_order(lib):
    none = {n: None for n in FWD_INPUTS}
    for kw in (dict(b=0), dict(L=0), dict(d=0), dict(rows=0), dict(q=0), dict(ld=19)):
        assert fwd(lib, q=kw.pop("q", 257), multiply=2, **none, **kw) == BAD_SHAPE, kw     # shape before limits
    for kw in (dict(q=257), dict(rows=257), dict(d=4097)):
        assert fwd(lib, multiply=2, **none, **kw) == Q_UNSUPPORTED, kw                      # limits before pointers
    for n in FWD_INPUTS:
        assert fwd(lib, multiply=2, **{n: None}) == NULL_POINTER, n                         # pointers before multiply
    for multiply in (2, -1):
        assert fwd(lib, multiply=multiply) == BAD_ARGUMENT, multiply


def test_backward_error_codes_in_order(lib):
    none = {n: None for n in GRAD_INPUTS}
    for kw in (dict(b=0), dict(L=0), dict(d=0), dict(rows=0), dict(q=0), dict(ld=19), dict(ldd=19)):
        assert grad(lib, q=kw.pop("q", 257), ws=None, nbytes=0, **none, **kw) == BAD_SHAPE, kw
    for kw in (dict(q=257), dict(rows=257), dict(d=4097)):
        assert grad(lib, ws=None, nbytes=0, **none, **kw) == Q_UNSUPPORTED, kw
    assert grad(lib, ws=None, nbytes=0, **none) == NULL_POINTER
    for n in GRAD_INPUTS:
        assert grad(lib, nbytes=0, **{n: None}) == NULL_POINTER, n                          # pointers before workspace
    assert grad(lib, ws=None) == NULL_POINTER
    assert grad(lib, nbytes=0, dE_in=None, demb=None, tabs=(None, None, None)) == NULL_POINTER   # no output at all
    for tabs in ((256, None, None), (None, 256, None), (None, None, 256), (256, 256, None), (256, None, 256),
                 (None, 256, 256)):
        assert grad(lib, nbytes=0, tabs=tabs) == NULL_POINTER, tabs
    assert grad(lib, nbytes=0, E_in=None) == NULL_POINTER                                   # dE_in without E_in
    need = lib.hmm_embedding_emissions_grad_wide_workspace_bytes(2, 300, 20, 37, 43)
    for kw in (dict(), dict(E_in=None, dE_in=None), dict(dE_in=None), dict(demb=None, ldd=0), dict(tabs=(None,) * 3),
               dict(dE_in=None, demb=None), dict(demb=None, tabs=(None,) * 3), dict(dE_in=None, tabs=(None,) * 3)):
        assert grad(lib, nbytes=0, **kw) == WORKSPACE, kw
        assert grad(lib, nbytes=need - 1, **kw) == WORKSPACE, kw                            # one byte short
        assert grad(lib, ws=256 + 8, nbytes=need + 256, **kw) == WORKSPACE, kw              # misaligned


def test_workspace_query(lib):
    wsb = lib.hmm_embedding_emissions_grad_wide_workspace_bytes
    dmax = lib.hmm_embedding_emissions_grad_max_dim()
    for dims in ((0, 5, 8, 37, 43), (2, 0, 8, 37, 43), (2, 5, 0, 37, 43), (2, 5, 8, 0, 43), (2, 5, 8, 37, 0),
                 (2, 5, 8, 257, 43), (2, 5, 8, 37, 257), (2, 5, dmax + 1, 37, 43)):
        assert wsb(*dims) == 0, dims
    for rows, q in ((1, 1), (3, 256), (37, 43), (61, 71), (253, 253), (256, 256), (40, 5), (32, 64)):
        for d in (1, 3, 16, 17, 64, 130, 256, 257, 1000, dmax):
            for b, L in ((1, 1), (2, 300), (64, 10000), (64, 1000000)):
                n = wsb(b, L, d, rows, q)
                w = b * L * ((rows + 3) // 4 * 4) * 4
                assert n > 0 and n % 256 == 0, (b, L, d, rows, q)
                assert w + rows * (2 * d + 1) * 4 <= n <= w + MIB16 + 512, (b, L, d, rows, q, n - w)
            # beyond W the workspace stops growing with b L
            big, bigger = wsb(64, 100000, d, rows, q), wsb(64, 1000000, d, rows, q)
            assert bigger - 64 * 1000000 * ((rows + 3) // 4 * 4) * 4 <= big - 64 * 100000 * ((rows + 3) // 4 * 4) * 4 + 256
    assert wsb(64, 1000000, 64, 256, 256) > 2 ** 32                                         # 64-bit sizes


def test_the_64_state_pair_keeps_its_limits(lib):
    assert fwd(lib, "hmm_embedding_emissions", q=64, rows=32, emb=None) == NULL_POINTER
    assert fwd(lib, "hmm_embedding_emissions", q=65, rows=32) == Q_UNSUPPORTED
    assert fwd(lib, "hmm_embedding_emissions", q=64, rows=33) == Q_UNSUPPORTED
    assert grad(lib, "hmm_embedding_emissions_grad", q=65, rows=32, nbytes=0) == Q_UNSUPPORTED
    assert grad(lib, "hmm_embedding_emissions_grad", q=64, rows=33, nbytes=0) == Q_UNSUPPORTED
    assert lib.hmm_embedding_emissions_grad_workspace_bytes(2, 3, 15, 32, 65) == 0
    assert lib.hmm_embedding_emissions_grad_workspace_bytes(2, 3, 15, 33, 64) == 0


def test_python_entry_points_have_no_cpu_path(lib):
    z = torch.zeros
    args = (z(2, 3, 30), 15, 8, z(37, 8), z(37, 8), z(37), z(43, dtype=torch.int32))
    with pytest.raises(engine.EngineError):
        engine.embedding_emissions_wide(*args)
    with pytest.raises(engine.EngineError):
        engine.embedding_emissions_grad_wide(*args, z(2, 3, 43))


def emitter(copies, shared=True, **kw):
    em = GenePredHMMEmitter(**CODONS, num_copies=copies, share_intron_parameters=shared, **kw)
    em.build((1, 2, 24, 15))
    return em


def test_routing_rules(lib):
    route = engine.embedding_emissions_routes_wide
    assert route(64, 32) is False and route(15, 13) is False and route(1, 1) is False
    assert route(65, 32) is True and route(64, 33) is True and route(256, 256) is True
    assert route(257, 1) is None and route(1, 257) is None
    emb = dict(emit_embeddings=True, embedding_dim=4)
    # (copies, shared introns) -> fused_routes() without / with embeddings, fused_route() without / with embeddings
    table = {(1, False): (("gene", None), ("gene", "mvn"), "gene", "gene"),         # 15 states
             (2, False): (("gene", None), ("gene", "mvn"), "gene", "gene"),         # 29 states and rows
             (3, False): (("wide", None), ("wide", "mvn_wide"), "wide", None),      # 43 states and rows
             (5, False): (("wide", None), ("wide", "mvn_wide"), "wide", None),      # 71
             (18, False): (("wide", None), ("wide", "mvn_wide"), "wide", None),     # 253
             (19, False): ((None, None), (None, None), None, None),                 # 267
             (3, True): (("wide", None), ("wide", "mvn_wide"), "wide", None),       # 43 states, 37 rows
             (5, True): (("wide", None), ("wide", "mvn_wide"), "wide", None),       # 71 states, 61 rows
             (19, True): ((None, None), (None, None), None, None)}
    x = torch.zeros(1, 2, 24, 20)
    for (copies, shared), (plain, with_emb, one_plain, one_emb) in table.items():
        a, b = emitter(copies, shared), emitter(copies, shared, **emb)
        assert a.fused_routes() == plain and b.fused_routes() == with_emb, (copies, shared)
        assert a.fused_route() == one_plain and b.fused_route() == one_emb, (copies, shared)      # unchanged
        assert a.can_fuse(x) is False and b.can_fuse(torch.zeros(1, 2, 24, 24)) is False           # never on CPU tensors


def test_row_block_formulation_equals_fp64_autograd():
    """The backward as the wide kernels organise it — rows in blocks of 32, the states of a block in chunks of 32
    taken from the row-sorted state list, W written per block, demb summed over all rows, the table sums per block —
    restated in fp64 torch, against autograd through the forward's formula."""
    g = torch.Generator().manual_seed(5)
    npos, d, rows, T, add = 11, 7, 70, 7.0, 1e-10
    row = torch.randint(0, rows, (90,), generator=g)
    row[:3] = torch.tensor([69, 0, 69])
    q = row.numel()
    leaf = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64).requires_grad_(True)
    emb, mean, log_norm = leaf(npos, d), leaf(rows, d), leaf(rows)
    inv_std = (0.5 + torch.rand(rows, d, generator=g, dtype=torch.float64)).requires_grad_(True)
    Ein = (0.5 + torch.rand(npos, q, generator=g, dtype=torch.float64)).requires_grad_(True)
    dE = torch.randn(npos, q, generator=g, dtype=torch.float64)
    lp = log_norm - 0.5 * torch.square((emb.unsqueeze(-2) - mean) * inv_std).sum(-1)
    ((Ein * (torch.exp(lp / T) + add)[..., row]) * dE).sum().backward()

    with torch.no_grad():
        order = sorted(range(q), key=lambda j: (int(row[j]), j))                    # rlist
        rstart = [sum(int(r) < k for r in row) for k in range(rows + 1)]
        gfn = torch.exp(lp / T)
        W = torch.zeros(npos, rows, dtype=torch.float64)
        dE_in = torch.full((npos, q), float("nan"), dtype=torch.float64)
        for r0 in range(0, rows, 32):
            r1 = min(r0 + 32, rows)
            Gf = torch.zeros(npos, rows, dtype=torch.float64)
            for kc in range(rstart[r0], rstart[r1], 32):
                for k in range(kc, min(kc + 32, rstart[r1])):
                    j = order[k]
                    assert r0 <= int(row[j]) < r1
                    dE_in[:, j] = dE[:, j] * (gfn[:, row[j]] + add)
                    Gf[:, row[j]] += dE[:, j] * Ein[:, j]
            W[:, r0:r1] = (Gf * gfn / T)[:, r0:r1]
        t = emb.unsqueeze(-2) - mean                                                # (npos, rows, d)
        demb = -(W.unsqueeze(-1) * t * inv_std ** 2).sum(1)
        dmean = (W.unsqueeze(-1) * t).sum(0) * inv_std ** 2
        dinv_std = -(W.unsqueeze(-1) * t * t).sum(0) * inv_std
        for got, want in ((dE_in, Ein.grad), (demb, emb.grad), (dmean, mean.grad), (dinv_std, inv_std.grad),
                          (W.sum(0), log_norm.grad)):
            assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
