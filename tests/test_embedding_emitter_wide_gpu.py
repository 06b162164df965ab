"""hmm_embedding_emissions_wide / hmm_embedding_emissions_grad_wide on a HIP device: the embedding factor and its
backward for up to 256 states and 256 kernel rows, from the kernels up to the layer.  Needs an MI355X.

Methods and bounds are those of tests/test_embedding_emitter_gpu.py and tests/test_embedding_emitter_grad_gpu.py,
unchanged, with the same input construction seeded the same way:
  forward   max rel err <= max(4 e32, max|log_pdf / T| 2^-24), every element compared, each case first asserting
            that its fp64 reference is >= 1e-30 (e32: the CPU fp32 torch path's error against fp64; the factor 4
            covers another summation order over d; the second term is the rounding of exp's fp32 argument);
  backward  per output tensor max|got - ref| <= max(4 e32, 2e-6 max|ref|, max|log_pdf / T| 2^-24 max|ref|) against
            fp64 CPU autograd, e32 from fp32 CPU autograd of the same case;
  layer     2e-5 on posteriors, 1e-6 |x| + 2e-4 on loglik and score, <= 1 % of path positions; a training step
            within 5e-4 scale + 1e-7 of fp64 CPU autograd.
Shapes: (3, 5), (4, 37) and (2, 300) — more than one tile of positions with a partial last one at any tile width up
to 256."""
import copy
import functools
import itertools

import pytest
import torch

from hmm_layer_amd import Viterbi, autograd, engine
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
SHAPES = [(3, 5), (4, 37), (2, 300)]
DIMS = [1, 3, 16, 17, 64, 130]


def shared_introns(c):
    """state -> kernel row of the c-copy model with shared introns, as GenePredHMMEmitter.state_tables builds it."""
    return list(range(1 + c)) + list(range(1, 1 + c)) * 2 + list(range(1 + c, 1 + 12 * c))


# name -> (rows, state_row)
WIDE = {"r33": (33, list(range(33))), "q43": (37, shared_introns(3)), "r65": (65, list(range(65))),
        "q71": (61, shared_introns(5)), "q253": (253, list(range(253))), "r256": (256, list(range(256))),
        "q256r3": (3, [j % 3 for j in range(256)]),                  # many states folding into one row
        "q5r40": (40, [39, 0, 17, 33, 39])}                           # rows the states never touch
BOTH = {"q15": (13, shared_introns(1)), "q29": (25, shared_introns(2)), "r32": (32, list(range(32)))}
ROWMAPS = dict(WIDE, **BOTH)
OUTPUTS = ("dE_in", "demb", "dmean", "dinv_std", "dlog_norm")
assert len(WIDE["q43"][1]) == 43 and len(WIDE["q71"][1]) == 71 and BOTH["q15"][1] == [0, 1, 1, 1] + list(range(2, 13))


def shell(d, ker):
    """An emitter object carrying a (rows, 2d) parameter: rows need not be a model's row count here."""
    em = SimpleGenePredHMMEmitter(emit_embeddings=True, embedding_dim=d)
    em.embedding_emission_kernel = torch.nn.Parameter(ker.reshape(1, ker.shape[0], 1, 2 * d).clone())
    return em


@functools.lru_cache(maxsize=None)
def reference(b, L, d, rowmap, far):
    """One (shape, d, row map, input kind), built once and shared: parameter, inputs, the fp64 log_pdf, the fp32
    torch path's log_pdf, the kernel's fp32 tables and an upstream gradient of mixed signs (CPU).  The construction
    and the seed of test_embedding_emitter_gpu.reference / test_embedding_emitter_grad_gpu.reference."""
    rows, state_row = ROWMAPS[rowmap]
    g = torch.Generator().manual_seed(100000 * int(far) + 1000 * b + 7 * L + 13 * d + rows)
    mean = torch.randn((rows, d), generator=g) + (30.0 if far else 0.0)
    ker = torch.cat([mean, 0.3 + 0.3 * torch.randn((rows, d), generator=g)], -1)
    if far:                 # every embedding next to row r0's mean: an expanded form would cancel here
        r0 = int(torch.randint(0, rows, (1,), generator=g))
        emb = mean[r0] + 0.1 * torch.randn((b, L, d), generator=g)
    else:
        emb = torch.randn((b, L, d), generator=g)
    em = shell(d, ker)
    em64 = copy.deepcopy(em).double()
    with torch.no_grad():
        em64.embedding_mu, em64.embedding_sigma = em64.make_mvn()
        lp64 = em64.embedding_log_pdf(emb.double())
        em.embedding_mu, em.embedding_sigma = em.make_mvn()
        lp32 = em.embedding_log_pdf(emb)
    Ein = 0.5 + torch.rand((b, L, len(state_row)), generator=g)
    dE = torch.randn((b, L, len(state_row)), generator=g)
    tables = em.embedding_tables(torch.device("cpu"))
    return dict(emb=emb, lp64=lp64, lp32=lp32, Ein=Ein, dE=dE, tables=tables,
                row=torch.tensor(state_row, dtype=torch.int32))


def device_inputs(c, d, s, fill=float("nan")):
    """x (b, L, s + d + 5) on the device, its other columns NaN, and the tables and row map."""
    b, L = c["emb"].shape[:2]
    x = torch.full((b, L, s + d + 5), fill)
    x[..., s:s + d] = c["emb"]
    return x.to(DEV), [t.to(DEV) for t in c["tables"]], c["row"].to(DEV)


def run_forward(c, d, s, T, add, multiply, fn=None):
    x, tables, row = device_inputs(c, d, s)
    E = c["Ein"].to(DEV).clone() if multiply else None
    out = (fn or engine.embedding_emissions_wide)(x, s, d, *tables, row, E=E, inv_temperature=1.0 / T, add=add)
    assert (out is E) if multiply else tuple(out.shape) == (*c["emb"].shape[:2], c["row"].numel())
    return out


# ------------------------------------------------------------------------------------------------ 1. forward

@pytest.mark.parametrize("b,L", SHAPES)
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("rowmap", list(WIDE))
def test_forward_against_fp64(rowmap, d, b, L):
    worst = 0.0
    for far in (False, True):
        c = reference(b, L, d, rowmap, far)
        idx = c["row"].long()
        for T in ([float(d), 1.0] if d <= 4 else [float(d)]):
            for add in (0.0, 1e-10):
                f64 = (torch.exp(c["lp64"] / T) + add)[..., idx]
                f32 = (torch.exp(c["lp32"] / T) + add)[..., idx]
                assert float(f64.min()) >= 1e-30, (far, T, float(f64.min()))
                floor = float((c["lp64"] / T).abs().max()) * 2.0 ** -24
                for multiply in (0, 1):
                    ref = f64 * c["Ein"].double() if multiply else f64
                    c32 = (f32 * c["Ein"] if multiply else f32).double()
                    e32 = float(((c32 - ref).abs() / ref).max())
                    bound = max(4 * e32, floor)
                    for s in (15, 16):
                        got = run_forward(c, d, s, T, add, multiply).cpu().double()
                        assert bool(torch.isfinite(got).all())
                        err = float(((got - ref).abs() / ref).max())
                        worst = max(worst, err / bound)
                        print("%s d=%d (%d,%d) far=%d T=%g add=%g mult=%d s=%d: min ref %.3g  e32 %.3g  floor %.3g  "
                              "kernel err %.3g" % (rowmap, d, b, L, far, T, add, multiply, s, float(ref.min()), e32,
                                                   floor, err))
                        assert err <= bound, (far, T, add, multiply, s, err, bound)
    print("worst err / bound %.3g" % worst)


# ------------------------------------------------------------------------------------------------ 2. bit-identity

@pytest.mark.parametrize("d", [3, 17, 64, 130])
@pytest.mark.parametrize("rowmap", list(BOTH))
def test_forward_is_bit_identical_to_the_64_state_kernel(rowmap, d):
    for b, L in SHAPES:
        c = reference(b, L, d, rowmap, False)
        for multiply in (0, 1):
            for add in (0.0, 1e-10):
                for T in ([float(d), 1.0] if d <= 4 else [float(d)]):
                    new = run_forward(c, d, 15, T, add, multiply)
                    old = run_forward(c, d, 15, T, add, multiply, fn=engine.embedding_emissions)
                    assert torch.equal(new, old), (b, L, multiply, add, T)
                    assert torch.equal(new, run_forward(c, d, 15, T, add, multiply)), "repeated call"


# ------------------------------------------------------------------------------------------------ 3. backward

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


def run_backward(c, d, s, T, add, multiply, dE=None, fn=None, **kw):
    x, tables, row = device_inputs(c, d, s)
    out = (fn or engine.embedding_emissions_grad_wide)(
        x, s, d, *tables, row, (c["dE"] if dE is None else dE).to(DEV), E_in=c["Ein"].to(DEV) if multiply else None,
        inv_temperature=1.0 / T, add=add, **kw)
    return dict(zip(OUTPUTS, out))


def check(got, ref, c32, floor, tag):
    """The backward bound of the module docstring for every output present in ref -> worst err / bound."""
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
@pytest.mark.parametrize("rowmap", list(WIDE))
def test_backward_against_fp64_autograd(rowmap, d, b, L):
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
                        x, tables, row = device_inputs(c, d, s)
                        dx = torch.full_like(x, float("nan"))          # demb through ldd into a NaN-filled tensor
                        out = engine.embedding_emissions_grad_wide(
                            x, s, d, *tables, row, c["dE"].to(DEV), E_in=c["Ein"].to(DEV) if multiply else None,
                            inv_temperature=1.0 / T, add=add, dx_out=dx)
                        got = dict(zip(OUTPUTS, out))
                        assert got["demb"] is dx
                        assert bool(torch.isnan(dx[..., :s]).all()) and bool(torch.isnan(dx[..., s + d:]).all())
                        got["demb"] = dx[..., s:s + d]
                        worst = max(worst, check(got, ref, c32, lpmax * 2.0 ** -24, tag))
    print("worst err / bound %.3g" % worst)


# ------------------------------------------------------------------------------------------------ 4. determinism

@pytest.mark.parametrize("rowmap,d", [("r33", 17), ("q43", 64), ("r65", 3), ("q71", 64), ("q253", 16), ("r256", 130),
                                      ("q256r3", 17), ("q5r40", 64)])
def test_output_subsets_and_repeated_calls_are_bit_identical(rowmap, d):
    c = reference(2, 300, d, rowmap, False)
    joint = run_backward(c, d, 15, float(d), 1e-10, 1)
    again = run_backward(c, d, 15, float(d), 1e-10, 1)
    for n in OUTPUTS:
        assert torch.equal(joint[n], again[n]), n
    groups = {"want_dE_in": ("dE_in",), "want_demb": ("demb",), "want_tables": ("dmean", "dinv_std", "dlog_norm")}
    for k in (1, 2):
        for on in itertools.combinations(groups, k):
            got = run_backward(c, d, 15, float(d), 1e-10, 1, **{w: w in on for w in groups})
            for w, names in groups.items():
                for n in names:
                    if w in on:
                        assert torch.equal(got[n], joint[n]), (on, n)
                    else:
                        assert got[n] is None, (on, n)
    none = run_backward(c, d, 15, float(d), 1e-10, 1, want_dE_in=False, want_demb=False, want_tables=False)
    assert all(v is None for v in none.values())


# ------------------------------------------------------------------------------------------------ 5. locality

@pytest.mark.parametrize("at", [0, 255, 256, 2 * 300 - 1])
def test_gradient_at_one_position_stays_there(at):
    b, L, d, s = 2, 300, 64, 15
    c = reference(b, L, d, "q43", False)
    where = divmod(at, L)
    dE = torch.zeros_like(c["dE"])
    dE[where] = c["dE"][where]
    x, tables, row = device_inputs(c, d, s)
    dx = torch.full_like(x, float("nan"))
    dE_in, demb, dmean, dinv_std, dlog_norm = engine.embedding_emissions_grad_wide(
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
    alone = engine.embedding_emissions_grad_wide(x, s, d, *tables, row, dE.to(DEV), E_in=c["Ein"].to(DEV),
                                                 inv_temperature=1.0 / d)[1]
    assert tuple(alone.shape) == (b, L, d) and torch.equal(alone.cpu(), dx[..., s:s + d])


# ------------------------------------------------------------------------------------------------ 6. graph capture

def test_graph_capture_replays_the_eager_result():
    b, L, d, s = 2, 300, 64, 15
    c = reference(b, L, d, "q43", False)
    x, tables, row = device_inputs(c, d, s)
    dE, Ein = c["dE"].to(DEV), c["Ein"].to(DEV)
    eager_f = engine.embedding_emissions_wide(x, s, d, *tables, row, E=Ein.clone(), inv_temperature=1.0 / d)
    eager_b = engine.embedding_emissions_grad_wide(x, s, d, *tables, row, dE, E_in=Ein, inv_temperature=1.0 / d, add=1e-10)
    static_f = Ein.clone()
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):          # one stream, no branches
            engine.embedding_emissions_wide(x, s, d, *tables, row, E=static_f, inv_temperature=1.0 / d)
            static_b = engine.embedding_emissions_grad_wide(x, s, d, *tables, row, dE, E_in=Ein,
                                                            inv_temperature=1.0 / d, add=1e-10)
    static_f.copy_(Ein)                                        # capture does not run the kernels; replay does
    for t in static_b:
        t.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(static_f, eager_f)
    for n, a, e in zip(OUTPUTS, static_b, eager_b):
        assert torch.equal(a, e), n


# ------------------------------------------------------------------------------------------------ 7. autograd node

NAMES = ("embedding_emissions", "embedding_emissions_wide", "embedding_emissions_grad", "embedding_emissions_grad_wide")


def spy(monkeypatch):
    """Counts the calls of the four engine wrappers -> dict name -> count."""
    calls = dict.fromkeys(NAMES, 0)

    def wrap(name):
        real = getattr(engine, name)

        def counted(*a, **k):
            calls[name] += 1
            return real(*a, **k)
        return counted

    for name in NAMES:
        monkeypatch.setattr(engine, name, wrap(name))
    return calls


@pytest.mark.parametrize("rowmap,wide", [("q43", True), ("q15", False)])
def test_autograd_node_picks_the_pair(rowmap, wide, monkeypatch):
    b, L, d, s, add = 2, 300, 17, 15, 1e-10
    T = float(d)
    c = reference(b, L, d, rowmap, True)
    ref, lpmax = torch_grads(c, T, add, 1, torch.float64)
    c32, _ = torch_grads(c, T, add, 1, torch.float32)
    x, tables, row = device_inputs(c, d, s, fill=0.25)
    x.requires_grad_(True)
    mean, inv_std, log_norm = (t.requires_grad_(True) for t in tables)
    Ein = c["Ein"].to(DEV).requires_grad_(True)
    fwd = engine.embedding_emissions_wide if wide else engine.embedding_emissions
    want = fwd(x.detach(), s, d, mean.detach(), inv_std.detach(), log_norm.detach(), row, E=Ein.detach().clone(),
               inv_temperature=1.0 / T, add=add)
    calls = spy(monkeypatch)
    out = autograd.embedding_emissions(Ein, x, mean, inv_std, log_norm, row, s, d, inv_temperature=1.0 / T, add=add)
    assert torch.equal(out.detach(), want) and torch.equal(Ein.detach().cpu(), c["Ein"])       # E_in survives
    (out * c["dE"].to(DEV)).sum().backward()
    w = "_wide" if wide else ""
    assert calls == {n: int(n in ("embedding_emissions" + w, "embedding_emissions_grad" + w)) for n in NAMES}, calls
    xg = x.grad.cpu()
    assert float(xg[..., :s].abs().max()) == 0.0 and float(xg[..., s + d:].abs().max()) == 0.0
    got = dict(dE_in=Ein.grad, demb=x.grad[..., s:s + d], dmean=mean.grad, dinv_std=inv_std.grad, dlog_norm=log_norm.grad)
    check(got, ref, c32, lpmax * 2.0 ** -24, "node %s" % rowmap)


# ------------------------------------------------------------------------------------------------ layer level

MODELS = {"c3_shared_d5": (dict(num_copies=3), 5),                                    # 43 states, 37 rows
          "c5_shared_d16": (dict(num_copies=5), 16),                                  # 71 states, 61 rows
          "c4_unshared_d4": (dict(num_copies=4, share_intron_parameters=False), 4),   # 57 states and rows
          "c3_shared_d64": (dict(num_copies=3), 64)}
S = 15


def make_inputs(b, L, d, g):
    cls = torch.softmax(2 * torch.randn((1, b, L, S), generator=g), -1)
    emb = torch.randn((1, b, L, d), generator=g)
    nuc = torch.nn.functional.one_hot(torch.randint(0, 5, (1, b, L), generator=g), 5).float()      # one-hot with N
    return torch.cat([cls, emb, nuc], -1)


def make_emitter(model, g, fused=False):
    kw, d = MODELS[model]
    em = GenePredHMMEmitter(**CODONS, **kw, emit_embeddings=True, embedding_dim=d, temperature=float(d),
                            fused_training=fused)
    em.build((1, 1, 1, S))
    with torch.no_grad():
        em.emission_kernel.copy_(torch.randn(em.emission_kernel.shape, generator=g))
        ker = torch.randn(em.embedding_emission_kernel.shape, generator=g)
        ker[..., d:] = 0.3 + 0.3 * ker[..., d:]
        em.embedding_emission_kernel.copy_(ker)
    return em, d


def gene_cell(model, b, L, seed, fused=False):
    g = torch.Generator().manual_seed(seed)
    em, d = make_emitter(model, g, fused)
    x = make_inputs(b, L, d, g)
    hints = 0.25 + 0.75 * torch.rand((1, b, 2, em.num_states), generator=g)
    tr = GenePredMultiHMMTransitioner(k=em.num_copies, initial_exon_len=200, initial_intron_len=4500,
                                      initial_ir_len=10000)
    return HmmCell([em.num_states], S, em, tr), x, hints


@pytest.mark.parametrize("model", ["c3_shared_d5", "c5_shared_d16", "c4_unshared_d4"])
def test_forward_fused_matches_the_fp64_module(model):
    b, L = 2, 300
    g = torch.Generator().manual_seed(50 * b + L + len(model))
    em, d = make_emitter(model, g)
    x = make_inputs(b, L, d, g)
    hints = torch.rand((1, b, 2, em.num_states), generator=g)
    em64 = copy.deepcopy(em).double()
    dev = copy.deepcopy(em).to(DEV)
    xd = x.to(DEV)
    assert dev.can_fuse(xd) and dev.fused_routes() == ("wide", "mvn_wide")
    for h in (None, hints):
        with torch.no_grad():
            em64.recurrent_init()
            ref = em64(x.double(), end_hints=None if h is None else h.double())
            em.recurrent_init()
            c32 = em(x, end_hints=h).double()
            dev.recurrent_init()
        got = dev.forward_fused(xd, end_hints=None if h is None else h.to(DEV))
        assert got.shape == (1, b, L, em.num_states) and not got.requires_grad
        got = got.cpu().double()
        nz = ref > 0                                           # 3-mer factors may be exactly 0, in every path
        assert bool((got[~nz] == 0).all()) and float(ref[nz].min()) >= 1e-30
        e32 = float(((c32 - ref).abs()[nz] / ref[nz]).max())
        with torch.no_grad():
            lp = em64.embedding_log_pdf(x.double()[0][..., S:S + d]) / d
        bound = max(4 * e32, float(lp.abs().max()) * 2.0 ** -24)
        err = float(((got - ref).abs()[nz] / ref[nz]).max())
        print("%s hints=%s: e32 %.3g  fused err %.3g  bound %.3g" % (model, h is not None, e32, err, bound))
        assert err <= bound, (err, bound)


@pytest.mark.parametrize("model", ["c3_shared_d5", "c5_shared_d16", "c4_unshared_d4"])
def test_layer_inference_through_the_fused_path(model, monkeypatch):
    b, L = 3, 450
    cell, x, _ = gene_cell(model, b, L, 21)
    cell, x = cell.to(DEV), x.to(DEV)
    em = cell.emitter[0]
    layer = MsaHmmLayer(cell, use_prior=False)
    layer.build(x.shape)
    calls = spy(monkeypatch)

    def run():
        with torch.no_grad():
            post = layer.state_posterior_log_probs(x)
            path, score = Viterbi.viterbi(x, cell)
            loglik, mean = layer(x)
        return post, path, score, loglik

    post, path, score, loglik = run()
    assert calls["embedding_emissions_wide"] == 3 and calls["embedding_emissions"] == 0     # every call: the wide kernel
    monkeypatch.setattr(em, "can_fuse", lambda inputs: False)  # the same calls through forward()
    post_t, path_t, score_t, loglik_t = run()
    assert calls["embedding_emissions_wide"] == 3
    q = em.num_states
    assert post.shape == (1, b, L, q) and path.shape == (1, b, L)
    assert float((post.exp() - post_t.exp()).abs().max()) <= 2e-5
    assert float((post.exp().sum(-1) - 1).abs().max()) <= 2e-5
    assert bool(((loglik - loglik_t).abs() <= 1e-6 * loglik_t.abs() + 2e-4).all())
    assert bool(((score - score_t).abs() <= 1e-6 * score_t.abs() + 2e-4).all())
    assert float((path != path_t).float().mean()) <= 0.01


@pytest.mark.parametrize("hints", [False, True])
@pytest.mark.parametrize("model", ["c3_shared_d5", "c5_shared_d16", "c4_unshared_d4"])
def test_layer_trains_through_the_wide_pair(model, hints, monkeypatch):
    """One training step through the layer with fused_training=True against fp64 CPU autograd through an fp64 copy
    of the module and the oracle's log-likelihood; the project's layer tolerance, 5e-4 scale + 1e-7."""
    b, L = 3, 60
    d = MODELS[model][1]
    calls = spy(monkeypatch)
    cell, x, h = gene_cell(model, b, L, 33, True)
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
    assert calls["embedding_emissions_wide"] >= 1 and calls["embedding_emissions_grad_wide"] == 1, calls
    assert calls["embedding_emissions"] == 0 and calls["embedding_emissions_grad"] == 0, calls
    got = {n: p.grad.detach().cpu().double() for n, p in cell.named_parameters() if p.grad is not None}
    gx = xd.grad.detach().cpu().double()
    loglik = loglik.detach().cpu().double().reshape(-1)

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
    pairs += [("x.grad classes", gx[..., :S], wx[..., :S]), ("x.grad embedding", gx[..., S:S + d], wx[..., S:S + d])]
    for n, g, w in pairs:
        scale = float(w.abs().max())
        err = float((g - w).abs().max())
        print("%s hints=%s %s: scale %.4g err %.3g" % (model, hints, n, scale, err))
        assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
        assert err <= 5e-4 * scale + 1e-7, (n, err, scale)
    assert float(gx[..., S + d:].abs().max()) == 0.0       # nucleotide columns: exactly 0


def test_fused_step_keeps_less_than_half_the_memory():
    """43 states, d = 64, b = 4, L = 2000.  The torch-op path keeps at least two (8000, 37, 64) fp32 tensors
    (152 MB); the fused path keeps tensors of size b L (s + d + 5) and b L q and a workspace of W + at most 16 MiB."""
    b, L = 4, 2000

    def peak(fused):
        cell, x, _ = gene_cell("c3_shared_d64", b, L, 7, fused)
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
