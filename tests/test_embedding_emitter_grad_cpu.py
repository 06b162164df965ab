"""Host side of hmm_embedding_emissions_grad (no device needed): the new symbols and limits, the workspace query, the
argument checks in their stated order, the backward formulas in fp64 torch against autograd through
embedding_log_pdf, and the table helper that keeps its graph."""
import copy
import math

import pytest
import torch

from hmm_layer_amd import build as hbuild
from hmm_layer_amd import engine
from hmm_layer_amd.gene_pred_hmm_emitter import SimpleGenePredHMMEmitter

OK, BAD_SHAPE, Q_UNSUPPORTED, NULL_POINTER, WORKSPACE = 0, -1, -2, -3, -4
INPUTS = ("emb", "mean", "inv_std", "log_norm", "state_row", "dE")


@pytest.fixture(scope="module")
def lib():
    hbuild.build()
    return engine.lib()


def call(lib, b=2, L=300, d=20, rows=13, q=15, ld=None, ldd=None, E_in=256, dE_in=256, demb=256, tabs=(256, 256, 256),
         ws=256, nbytes=None, **inputs):
    """hmm_embedding_emissions_grad with placeholder device pointers: every call here returns before any HIP call."""
    p = {n: inputs.get(n, 256) for n in INPUTS}
    if nbytes is None:
        nbytes = lib.hmm_embedding_emissions_grad_workspace_bytes(b, L, d, rows, q)
    return lib.hmm_embedding_emissions_grad(p["emb"], d + 20 if ld is None else ld, b, L, d, p["mean"], p["inv_std"],
                                            p["log_norm"], rows, p["state_row"], q, 1.0, 0.0, E_in, p["dE"], dE_in,
                                            demb, d if ldd is None else ldd, *tabs, ws, nbytes, None)


def test_symbols_and_limits(lib):
    for name in ("hmm_embedding_emissions_grad_max_dim", "hmm_embedding_emissions_grad_workspace_bytes",
                 "hmm_embedding_emissions_grad"):
        assert hasattr(lib, name), name
    assert 512 <= lib.hmm_embedding_emissions_grad_max_dim() <= lib.hmm_embedding_emissions_max_dim() == 4096
    assert lib.hmm_abi_version() == 3 == engine.ABI_VERSION


def test_workspace_query(lib):
    dmax = lib.hmm_embedding_emissions_grad_max_dim()
    for dims in ((0, 5, 8, 13, 15), (2, 0, 8, 13, 15), (2, 5, 0, 13, 15), (2, 5, 8, 0, 15), (2, 5, 8, 13, 0),
                 (2, 5, 8, 33, 15), (2, 5, 8, 13, 65), (2, 5, dmax + 1, 13, 15)):
        assert lib.hmm_embedding_emissions_grad_workspace_bytes(*dims) == 0, dims
    for b, L in ((1, 1), (2, 1100), (64, 10000)):
        for q in (1, 15, 64):
            last = 0
            for rows in (1, 4, 5, 13, 25, 32):
                n = lib.hmm_embedding_emissions_grad_workspace_bytes(b, L, 64, rows, q)
                assert n > 0 and n % 256 == 0 and n >= last, (b, L, rows, q, n, last)
                assert n >= b * L * rows * 4                                  # W
                last = n
            last = 0
            for d in (1, 3, 16, 17, 64, 130, 256, 257, 512, 1000, dmax):
                n = lib.hmm_embedding_emissions_grad_workspace_bytes(b, L, d, 32, q)
                assert n > 0 and n % 256 == 0 and n >= last, (b, L, d, q, n, last)
                last = n
    # the partials stop growing with b L: beyond W, at most 16 MiB
    for d, rows in ((64, 13), (dmax, 32)):
        n = lib.hmm_embedding_emissions_grad_workspace_bytes(64, 1000000, d, rows, 15)
        w = 64 * 1000000 * ((rows + 3) // 4 * 4) * 4
        assert w <= n <= w + (16 << 20) + 512, (d, rows, n - w)
        assert rows < 32 or n > 2 ** 32                                       # 64-bit sizes


def test_error_codes_in_order(lib):
    none = {n: None for n in INPUTS}
    dmax = lib.hmm_embedding_emissions_grad_max_dim()
    # shape first
    for kw in (dict(b=0), dict(L=0), dict(d=0), dict(rows=0), dict(q=0), dict(ld=19), dict(ldd=19)):
        assert call(lib, q=kw.pop("q", 65), ws=None, nbytes=0, **none, **kw) == BAD_SHAPE, kw
    # limits before pointers
    for kw in (dict(q=65), dict(rows=33), dict(d=dmax + 1)):
        assert call(lib, ws=None, nbytes=0, **none, **kw) == Q_UNSUPPORTED, kw
    # pointers before workspace
    assert call(lib, ws=None, nbytes=0, **none) == NULL_POINTER
    for n in INPUTS:
        assert call(lib, nbytes=0, **{n: None}) == NULL_POINTER, n
    assert call(lib, ws=None) == NULL_POINTER
    assert call(lib, nbytes=0, dE_in=None, demb=None, tabs=(None, None, None)) == NULL_POINTER       # no output at all
    for tabs in ((256, None, None), (None, 256, None), (None, None, 256), (256, 256, None), (256, None, 256),
                 (None, 256, 256)):
        assert call(lib, nbytes=0, tabs=tabs) == NULL_POINTER, tabs
    assert call(lib, nbytes=0, E_in=None) == NULL_POINTER                    # dE_in without E_in
    # workspace last; every subset of the outputs gets that far
    need = lib.hmm_embedding_emissions_grad_workspace_bytes(2, 300, 20, 13, 15)
    for kw in (dict(), dict(E_in=None, dE_in=None), dict(dE_in=None), dict(demb=None, ldd=0), dict(tabs=(None,) * 3),
               dict(dE_in=None, demb=None), dict(demb=None, tabs=(None,) * 3), dict(dE_in=None, tabs=(None,) * 3)):
        assert call(lib, nbytes=0, **kw) == WORKSPACE, kw
        assert call(lib, nbytes=need - 1, **kw) == WORKSPACE, kw
        assert call(lib, ws=256 + 8, nbytes=need + 256, **kw) == WORKSPACE, kw       # misaligned


def test_python_entry_point_has_no_cpu_path(lib):
    z = torch.zeros
    with pytest.raises(engine.EngineError):
        engine.embedding_emissions_grad(z(2, 3, 30), 15, 8, z(5, 8), z(5, 8), z(5), z(5, dtype=torch.int32), z(2, 3, 5))


def test_formulas_equal_fp64_autograd():
    """The formulas of hmm_emitter_mvn_grad.inc written out in fp64 torch against fp64 autograd through
    embedding_log_pdf: pins the signs and g (not f) in W independently of the kernel."""
    g = torch.Generator().manual_seed(5)
    b, L, d, rows, T, add = 2, 7, 5, 4, 3.0, 0.25          # a large add: g and f differ visibly
    state_row = torch.tensor([0, 1, 1, 2, 3, 3, 1])
    ker = torch.cat([torch.randn((rows, d), generator=g), 0.3 + 0.3 * torch.randn((rows, d), generator=g)], -1).double()
    em = SimpleGenePredHMMEmitter(emit_embeddings=True, embedding_dim=d, temperature=T).double()
    em.embedding_emission_kernel = torch.nn.Parameter(ker.reshape(1, rows, 1, 2 * d))
    x = torch.randn((b, L, d), generator=g).double().requires_grad_(True)
    E_in = (0.5 + torch.rand((b, L, 7), generator=g)).double().requires_grad_(True)
    dE = torch.randn((b, L, 7), generator=g).double()
    # autograd, with the tables as leaves
    mu, sigma = (t.detach() for t in em.make_mvn())
    mean = mu.clone().requires_grad_(True)
    inv_std = (1.0 / sigma).requires_grad_(True)
    log_norm = (-0.5 * d * math.log(2 * math.pi) - torch.log(sigma).sum(-1)).requires_grad_(True)
    md = (((x.unsqueeze(-2) - mean) * inv_std) ** 2).sum(-1)
    lp = log_norm - 0.5 * md
    em.embedding_mu, em.embedding_sigma = mu, sigma
    assert torch.allclose(lp.detach(), em.embedding_log_pdf(x.detach()), rtol=1e-12, atol=1e-12)
    out = E_in * (torch.exp(lp / T) + add)[..., state_row]
    (out * dE).sum().backward()
    # the formulas
    with torch.no_grad():
        gg = torch.exp(lp / T)
        f = gg + add
        Gf = torch.zeros_like(gg).index_add_(-1, state_row, dE * E_in)
        W = Gf * gg / T
        diff = x.unsqueeze(-2) - mean                                   # (b, L, rows, d)
        want = dict(dE_in=dE * f[..., state_row], dlog_norm=W.sum((0, 1)),
                    dmean=(W[..., None] * diff * inv_std ** 2).sum((0, 1)),
                    dinv_std=-(W[..., None] * diff ** 2 * inv_std).sum((0, 1)),
                    demb=-(W[..., None] * diff * inv_std ** 2).sum(-2))
    got = dict(dE_in=E_in.grad, dlog_norm=log_norm.grad, dmean=mean.grad, dinv_std=inv_std.grad, demb=x.grad)
    for n in want:
        assert float(got[n].abs().max()) > 0
        assert torch.allclose(want[n], got[n], rtol=1e-11, atol=1e-13), n
    # with f in place of g the table gradients would be off by add * Gf / T: visibly different here
    assert not torch.allclose((Gf * f / T).sum((0, 1)), log_norm.grad, rtol=1e-3)


def test_tables_with_graph():
    g = torch.Generator().manual_seed(9)
    d = 6
    em = SimpleGenePredHMMEmitter(emit_embeddings=True, embedding_dim=d, initial_variance=0.7)
    em.build((1, 1, 1, 15))
    rows = em.kernel_rows()
    with torch.no_grad():
        em.embedding_emission_kernel.copy_(torch.randn(em.embedding_emission_kernel.shape, generator=g))
    plain = em.embedding_tables(torch.device("cpu"))
    graph = em.embedding_tables_with_graph(torch.device("cpu"))
    for a, t in zip(plain, graph):
        assert t.dtype == torch.float32 and t.requires_grad and not a.requires_grad
        assert torch.equal(a, t.detach())
    assert tuple(graph[0].shape) == (rows, d) == tuple(graph[1].shape) and tuple(graph[2].shape) == (rows,)
    cm, cs, cl = (torch.randn(t.shape, generator=g) for t in graph)
    (graph[0] * cm).sum().add((graph[1] * cs).sum()).add((graph[2] * cl).sum()).backward()
    got = em.embedding_emission_kernel.grad.double()
    # the same chain through make_mvn in fp64
    em64 = copy.deepcopy(em).double()
    em64.zero_grad()
    mu, sigma = em64.make_mvn()
    log_norm = -0.5 * d * math.log(2 * math.pi) - torch.log(sigma).sum(-1)
    ((mu * cm.double()).sum() + ((1.0 / sigma) * cs.double()).sum() + (log_norm * cl.double()).sum()).backward()
    want = em64.embedding_emission_kernel.grad
    assert float(want.abs().max()) > 0
    assert float((got - want).abs().max()) <= 1e-6 * float(want.abs().max())
