"""hmm_embedding_emissions_grad on a HIP device: the backward of the embedding-emission factor against fp64 CPU
autograd, its output switches, locality, graph capture, the autograd node, and the layer trained through it.
Needs an MI355X.

Tolerance of the kernel and node tests, per output tensor (dE_in, demb, dmean, dinv_std, dlog_norm):
max|got - ref| <= max(4 e32, 2e-6 max|ref|, max|log_pdf / T| 2^-24 max|ref|).  e32 is the error of the same
computation done by fp32 CPU torch autograd against fp64 (test_emitter_grad_gpu's rule: the factor 4 covers another
summation order, nothing else); the third term is the rounding of exp's fp32 argument itself
(test_embedding_emitter_gpu's floor).  The reference differentiates E_in (exp(lp / T) + add)[..., row] with the
kernel's own fp32 tables as leaves."""
import copy
import functools
import itertools

import pytest
import torch

from hmm_layer_amd import autograd, engine
from hmm_layer_amd.MsaHmmCell import HmmCell
from hmm_layer_amd.MsaHMMLayer import MsaHmmLayer, _loglik_impl
from hmm_layer_amd.gene_pred_hmm_emitter import GenePredHMMEmitter, SimpleGenePredHMMEmitter
from hmm_layer_amd.gene_pred_hmm_transitioner import GenePredMultiHMMTransitioner
from oracle import torch64

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CODONS = dict(start_codons=[("ATG", 1.)], stop_codons=[("TAG", .34), ("TAA", .33), ("TGA", .33)],
              intron_begin_pattern=[("NGT", .99), ("NGC", .005), ("NAT", .005)],
              intron_end_pattern=[("AGN", .99), ("ACN", .01)])
SHAPES = [(3, 5), (7, 16), (4, 37), (2, 1100)]
DIMS = [1, 3, 4, 16, 17, 64, 130]
# name -> (rows, state_row): q = rows, and the shared-intron maps of the 15- and 29-state models
ROWMAPS = {"r5": (5, list(range(5))), "r32": (32, list(range(32))),
           "q15": (13, [0, 1, 1, 1] + list(range(2, 13))),
           "q29": (25, [0, 1, 2, 1, 2, 1, 2] + list(range(3, 25)))}
OUTPUTS = ("dE_in", "demb", "dmean", "dinv_std", "dlog_norm")


def shell(d, ker):
    """An emitter object carrying a (rows, 2d) parameter: rows need not be a model's row count here."""
    em = SimpleGenePredHMMEmitter(emit_embeddings=True, embedding_dim=d)
    em.embedding_emission_kernel = torch.nn.Parameter(ker.reshape(1, ker.shape[0], 1, 2 * d).clone())
    return em


@functools.lru_cache(maxsize=None)
def reference(b, L, d, rowmap, far):
    """One (shape, d, rows, input kind): the inputs of test_embedding_emitter_gpu.reference, the kernel's fp32
    tables and an upstream gradient of mixed signs (CPU)."""
    rows, state_row = ROWMAPS[rowmap]
    g = torch.Generator().manual_seed(100000 * int(far) + 1000 * b + 7 * L + 13 * d + rows)
    mean = torch.randn((rows, d), generator=g) + (30.0 if far else 0.0)
    ker = torch.cat([mean, 0.3 + 0.3 * torch.randn((rows, d), generator=g)], -1)
    if far:                 # every embedding next to row r0's mean: an expanded form would cancel here
        r0 = int(torch.randint(0, rows, (1,), generator=g))
        emb = mean[r0] + 0.1 * torch.randn((b, L, d), generator=g)
    else:
        emb = torch.randn((b, L, d), generator=g)
    Ein = 0.5 + torch.rand((b, L, len(state_row)), generator=g)
    dE = torch.randn((b, L, len(state_row)), generator=g)
    tables = shell(d, ker).embedding_tables(torch.device("cpu"))
    return dict(emb=emb, Ein=Ein, dE=dE, tables=tables, row=torch.tensor(state_row, dtype=torch.int32))


def torch_grads(c, T, add, multiply, dtype, dE=None):
    """Autograd through E_in (exp(lp / T) + add)[..., row] in `dtype` on the CPU -> (the five gradients as fp64,
    max|lp / T|)."""
    def leaf(t):                                    # a fresh leaf: the shared reference tensors stay as they are
        return t.detach().to(dtype).clone().requires_grad_(True)

    emb, Ein = leaf(c["emb"]), leaf(c["Ein"])
    mean, inv_std, log_norm = (leaf(t) for t in c["tables"])
    lp = log_norm - 0.5 * torch.square((emb.unsqueeze(-2) - mean) * inv_std).sum(-1)
    f = (torch.exp(lp / T) + add)[..., c["row"].long()]
    out = Ein * f if multiply else f
    (out * (c["dE"] if dE is None else dE).to(dtype)).sum().backward()
    grads = dict(dE_in=Ein.grad if multiply else None, demb=emb.grad, dmean=mean.grad, dinv_std=inv_std.grad,
                 dlog_norm=log_norm.grad)
    return {n: None if v is None else v.double() for n, v in grads.items()}, float((lp.detach() / T).abs().max())


def device_inputs(c, d, s, fill=float("nan")):
    """x (b, L, s + d + 5) on the device, its other columns NaN, and the tables and row map."""
    b, L = c["emb"].shape[:2]
    x = torch.full((b, L, s + d + 5), fill)
    x[..., s:s + d] = c["emb"]
    return x.to(DEV), [t.to(DEV) for t in c["tables"]], c["row"].to(DEV)


def run_kernel(c, d, s, T, add, multiply, dE=None, **kw):
    x, tables, row = device_inputs(c, d, s)
    out = engine.embedding_emissions_grad(x, s, d, *tables, row, (c["dE"] if dE is None else dE).to(DEV),
                                          E_in=c["Ein"].to(DEV) if multiply else None, inv_temperature=1.0 / T,
                                          add=add, **kw)
    return dict(zip(OUTPUTS, out))


def check(got, ref, c32, floor, tag):
    """The bound of the module docstring for every output present in ref -> worst err / bound."""
    worst = 0.0
    for n in OUTPUTS:
        if ref[n] is None:
            assert got[n] is None, n
            continue
        g = got[n].cpu().double()
        assert g.shape == ref[n].shape and bool(torch.isfinite(g).all()), (tag, n)
        scale = float(ref[n].abs().max())
        e32 = float((c32[n] - ref[n]).abs().max())
        err = float((g - ref[n]).abs().max())
        bound = max(4 * e32, 2e-6 * scale, floor * scale)
        worst = max(worst, err / bound)
        print("%s %s: max|ref| %.4g  e32 %.3g  err %.3g  bound %.3g" % (tag, n, scale, e32, err, bound))
        assert scale > 0
        assert err <= bound, (tag, n, err, bound)
    return worst


@pytest.mark.parametrize("b,L", SHAPES)
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("rowmap", list(ROWMAPS))
def test_kernel_against_fp64_autograd(rowmap, d, b, L):
    worst = 0.0
    for far in (False, True):
        c = reference(b, L, d, rowmap, far)
        for T in ([float(d), 1.0] if d <= 4 else [float(d)]):
            for add in (0.0, 1e-10):
                for multiply in (0, 1):
                    ref, lpmax = torch_grads(c, T, add, multiply, torch.float64)
                    c32, _ = torch_grads(c, T, add, multiply, torch.float32)
                    for s in (15, 16):
                        tag = "%s d=%d (%d,%d) far=%d T=%g add=%g mult=%d s=%d" % (rowmap, d, b, L, far, T, add, multiply, s)
                        worst = max(worst, check(run_kernel(c, d, s, T, add, multiply), ref, c32, lpmax * 2.0 ** -24, tag))
    print("worst err / bound %.3g" % worst)


@pytest.mark.parametrize("rowmap,d,b,L", [("q15", 64, 2, 1100), ("r32", 130, 4, 37), ("q29", 17, 7, 16)])
def test_output_subsets_and_repeated_calls_are_bit_identical(rowmap, d, b, L):
    c = reference(b, L, d, rowmap, False)
    joint = run_kernel(c, d, 15, float(d), 1e-10, 1)
    again = run_kernel(c, d, 15, float(d), 1e-10, 1)
    for n in OUTPUTS:
        assert torch.equal(joint[n], again[n]), n
    groups = {"want_dE_in": ("dE_in",), "want_demb": ("demb",), "want_tables": ("dmean", "dinv_std", "dlog_norm")}
    for k in (1, 2):
        for on in itertools.combinations(groups, k):
            got = run_kernel(c, d, 15, float(d), 1e-10, 1, **{w: w in on for w in groups})
            for w, names in groups.items():
                for n in names:
                    if w in on:
                        assert torch.equal(got[n], joint[n]), (on, n)
                    else:
                        assert got[n] is None, (on, n)
    none = run_kernel(c, d, 15, float(d), 1e-10, 1, want_dE_in=False, want_demb=False, want_tables=False)
    assert all(v is None for v in none.values())


@pytest.mark.parametrize("at", [0, 255, 256, 2 * 1100 - 1])
def test_gradient_at_one_position_stays_there(at):
    b, L, d, s = 2, 1100, 64, 15
    c = reference(b, L, d, "q15", False)
    where = divmod(at, L)
    dE = torch.zeros_like(c["dE"])
    dE[where] = c["dE"][where]
    x, tables, row = device_inputs(c, d, s)
    dx = torch.full_like(x, float("nan"))
    dE_in, demb, dmean, dinv_std, dlog_norm = engine.embedding_emissions_grad(
        x, s, d, *tables, row, dE.to(DEV), E_in=c["Ein"].to(DEV), inv_temperature=1.0 / d, dx_out=dx)
    assert demb is dx
    dx = dx.cpu()
    assert bool(torch.isnan(dx[..., :s]).all()) and bool(torch.isnan(dx[..., s + d:]).all())     # untouched columns
    for t in (dx[..., s:s + d], dE_in.cpu()):
        nz = t.abs().sum(-1)
        assert bool(torch.isfinite(t).all()) and float(nz[where]) > 0
        nz[where] = 0
        assert float(nz.max()) == 0.0
    for t in (dmean, dinv_std, dlog_norm):
        assert bool(torch.isfinite(t).all()) and float(t.abs().max()) > 0
    # the same gradient through a tensor of its own
    alone = engine.embedding_emissions_grad(x, s, d, *tables, row, dE.to(DEV), E_in=c["Ein"].to(DEV),
                                            inv_temperature=1.0 / d)[1]
    assert tuple(alone.shape) == (b, L, d) and torch.equal(alone.cpu(), dx[..., s:s + d])


def test_graph_capture_replays_the_eager_result():
    b, L, d, s = 2, 1100, 64, 15
    c = reference(b, L, d, "q15", False)
    x, tables, row = device_inputs(c, d, s)
    dE, Ein = c["dE"].to(DEV), c["Ein"].to(DEV)
    eager = engine.embedding_emissions_grad(x, s, d, *tables, row, dE, E_in=Ein, inv_temperature=1.0 / d, add=1e-10)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):          # one stream, no branches
            static = engine.embedding_emissions_grad(x, s, d, *tables, row, dE, E_in=Ein, inv_temperature=1.0 / d,
                                                     add=1e-10)
    for t in static:
        t.fill_(float("nan"))                                  # capture does not run the kernels; replay does
    graph.replay()
    torch.cuda.synchronize()
    for n, a, e in zip(OUTPUTS, static, eager):
        assert torch.equal(a, e), n


@pytest.mark.parametrize("ein_grad", [True, False])
@pytest.mark.parametrize("rowmap,d,b,L,far", [("q15", 64, 2, 1100, True), ("q29", 17, 4, 37, False)])
def test_autograd_node(rowmap, d, b, L, far, ein_grad):
    s, T, add = 15, float(d), 1e-10
    c = reference(b, L, d, rowmap, far)
    ref, lpmax = torch_grads(c, T, add, 1, torch.float64)
    c32, _ = torch_grads(c, T, add, 1, torch.float32)
    x, tables, row = device_inputs(c, d, s, fill=0.25)
    x.requires_grad_(True)
    mean, inv_std, log_norm = (t.requires_grad_(True) for t in tables)
    Ein = c["Ein"].to(DEV).requires_grad_(ein_grad)
    out = autograd.embedding_emissions(Ein, x, mean, inv_std, log_norm, row, s, d, inv_temperature=1.0 / T, add=add)
    want = engine.embedding_emissions(x.detach(), s, d, mean.detach(), inv_std.detach(), log_norm.detach(), row,
                                      E=Ein.detach().clone(), inv_temperature=1.0 / T, add=add)
    assert torch.equal(out.detach(), want) and torch.equal(Ein.detach().cpu(), c["Ein"])       # E_in survives
    (out * c["dE"].to(DEV)).sum().backward()
    assert (Ein.grad is not None) == ein_grad
    xg = x.grad.cpu()
    assert float(xg[..., :s].abs().max()) == 0.0 and float(xg[..., s + d:].abs().max()) == 0.0
    got = dict(dE_in=Ein.grad, demb=x.grad[..., s:s + d], dmean=mean.grad, dinv_std=inv_std.grad, dlog_norm=log_norm.grad)
    if not ein_grad:
        ref["dE_in"] = None
    check(got, ref, c32, lpmax * 2.0 ** -24, "node %s d=%d (%d,%d) E_in.grad=%s" % (rowmap, d, b, L, ein_grad))


# ------------------------------------------------------------------------------------------------ layer level

def make_inputs(b, L, s, d, g):
    cls = torch.softmax(2 * torch.randn((1, b, L, s), generator=g), -1)
    emb = torch.randn((1, b, L, d), generator=g)
    nuc = torch.nn.functional.one_hot(torch.randint(0, 5, (1, b, L), generator=g), 5).float()      # one-hot with N
    return torch.cat([cls, emb, nuc], -1)


MODELS = {"q15_d16": (1, 16), "q29_d5": (2, 5), "q15_d64": (1, 64)}             # name -> (copies, d)


def gene_cell(model, b, L, seed, fused):
    copies, d = MODELS[model]
    g = torch.Generator().manual_seed(seed)
    em = GenePredHMMEmitter(**CODONS, num_copies=copies, emit_embeddings=True, embedding_dim=d, temperature=float(d),
                            fused_training=fused)
    em.build((1, 1, 1, 15))
    with torch.no_grad():
        em.emission_kernel.copy_(torch.randn(em.emission_kernel.shape, generator=g))
        ker = torch.randn(em.embedding_emission_kernel.shape, generator=g)
        ker[..., d:] = 0.3 + 0.3 * ker[..., d:]
        em.embedding_emission_kernel.copy_(ker)
    x = make_inputs(b, L, 15, d, g)
    hints = 0.25 + 0.75 * torch.rand((1, b, 2, em.num_states), generator=g)
    kw = dict(k=copies) if copies > 1 else {}
    tr = GenePredMultiHMMTransitioner(initial_exon_len=200, initial_intron_len=4500, initial_ir_len=10000, **kw)
    return HmmCell([em.num_states], 15, em, tr), x, hints


def spy(monkeypatch):
    calls = []
    real = engine.embedding_emissions_grad
    monkeypatch.setattr(engine, "embedding_emissions_grad", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    return calls


@pytest.mark.parametrize("hints", [False, True])
@pytest.mark.parametrize("model", ["q15_d16", "q29_d5"])
def test_layer_trains_through_the_fused_embedding_backward(model, hints, monkeypatch):
    """One training step through the layer with fused_training=True against fp64 CPU autograd through an fp64 copy
    of the module and the oracle's log-likelihood (the protocol and tolerance of
    test_embedding_emitter_gpu.test_layer_trains_the_embedding_kernel: 5e-4 scale + 1e-7)."""
    b, L, s = 3, 60, 15
    d = MODELS[model][1]
    calls = spy(monkeypatch)

    def device_step(fused):
        cell, x, h = gene_cell(model, b, L, 33, fused)
        cell, xd = cell.to(DEV), x.to(DEV).requires_grad_(True)
        assert cell.emitter[0].can_fuse(xd)
        layer = MsaHmmLayer(cell, use_prior=False)
        layer.build(xd.shape)
        if hints:                                       # MsaHmmLayer.forward takes no end hints: the function under it
            loglik = _loglik_impl(xd, cell, end_hints=h.to(DEV), training=True)
        else:
            loglik = layer(xd, training=True)[0]
        (-loglik.mean()).backward()
        torch.cuda.synchronize()
        grads = {n: p.grad.detach().cpu().double() for n, p in cell.named_parameters() if p.grad is not None}
        return loglik.detach().cpu().double().reshape(-1), grads, xd.grad.detach().cpu().double()

    loglik, got, gx = device_step(True)
    assert len(calls) == 1                                  # the fused backward ran
    device_step(False)
    assert len(calls) == 1                                  # and the torch-op path does not call it

    cpu, x, h = gene_cell(model, b, L, 33, False)          # same seed: identical parameters
    cpu = cpu.double()
    x64 = x.double().requires_grad_(True)
    cpu.recurrent_init()
    E = cpu.emission_probs(x64, end_hints=h.double() if hints else None, training=True)[0]
    _, ll = torch64.posterior(cpu.A[0], cpu.init_dist.reshape(-1), E, eps=cpu.epsilon)
    (-ll.mean()).backward()
    assert bool(((loglik - ll.detach()).abs() <= 1e-6 * ll.detach().abs() + 2e-3).all())
    want = dict(cpu.named_parameters())
    pairs = [(n, got[n], want[n].grad) for n in ("emitter.0.embedding_emission_kernel", "emitter.0.emission_kernel")]
    wx = x64.grad
    pairs += [("x.grad classes", gx[..., :s], wx[..., :s]), ("x.grad embedding", gx[..., s:s + d], wx[..., s:s + d])]
    for n, g, w in pairs:
        scale = float(w.abs().max())
        err = float((g - w).abs().max())
        print("%s hints=%s %s: scale %.4g err %.3g" % (model, hints, n, scale, err))
        assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
        assert err <= 5e-4 * scale + 1e-7, (n, err, scale)
    assert float(gx[..., s + d:].abs().max()) == 0.0       # nucleotide columns: exactly 0


def test_fused_step_keeps_less_than_half_the_memory():
    """15 states, d = 64, b = 4, L = 5000.  The torch-op path keeps at least two (b L, 13, 64) fp32 tensors (133 MB);
    the fused path keeps tensors of size b L (s + d + 5) and b L q only (under 25 MB)."""
    b, L = 4, 5000

    def peak(fused):
        cell, x, _ = gene_cell("q15_d64", b, L, 7, fused)
        cell, x = cell.to(DEV), x.to(DEV)
        layer = MsaHmmLayer(cell, use_prior=False)
        layer.build(x.shape)

        def step():
            xs = x.clone().requires_grad_(True)
            cell.zero_grad(set_to_none=True)
            (-layer(xs, training=True)[1]).backward()
            torch.cuda.synchronize()
            return xs.grad

        step()                                              # the workspaces are cached from here on
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        gx = step()
        assert bool(torch.isfinite(gx).all())
        return torch.cuda.max_memory_allocated() - base

    fused, plain = peak(True), peak(False)
    print("peak bytes above the pre-step level: fused %d, torch ops %d" % (fused, plain))
    assert 2 * fused <= plain, (fused, plain)
