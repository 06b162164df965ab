"""hmm_nucleotide_emissions / hmm_nucleotide_emissions_grad on a HIP device: the two kernels against an fp64
restatement of the factor, their determinism and graph capture, the emitter's fused paths with
trainable_nucleotides_at_exons=True against forward(), and the layer.  Needs an MI355X.

Bound of the elementwise kernel tests: relative error <= 8 * 2^-24 against the fp64 evaluation of the same fp32 inputs
wherever that is non-zero, exact 0 where it is zero.  Every term of the factor is non-negative, so nothing cancels, and a
value goes through at most six rounded operations: the acgt add, one multiply and three fused multiply-adds, and the
product with E_in (dE for the backward).  dP and the module's parameter gradients go by the gradient rule of
test_emitter_grad_gpu: max|got - ref| <= max(4 e32, 2e-6 max|ref|), e32 the error of the fp32 torch path on the CPU."""
import copy
import functools

import pytest
import torch

from hmm_layer_amd import Viterbi, engine
from hmm_layer_amd.MsaHmmCell import HmmCell
from hmm_layer_amd.MsaHMMLayer import MsaHmmLayer
from hmm_layer_amd.gene_pred_hmm_emitter import GenePredHMMEmitter
from hmm_layer_amd.gene_pred_hmm_transitioner import GenePredMultiHMMTransitioner
from oracle import torch64

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CODONS = dict(start_codons=[("ATG", 1.)], stop_codons=[("TAG", .34), ("TAA", .33), ("TGA", .33)],
              intron_begin_pattern=[("NGT", .99), ("NGC", .005), ("NAT", .005)],
              intron_end_pattern=[("AGN", .99), ("ACN", .01)])
EPS = 8 * 2.0 ** -24
# one position, a ragged last tile, several tiles, a tile boundary inside a sequence
SHAPES = [(1, 1), (3, 5), (7, 16), (4, 37), (2, 1100), (5, 4099)]


def gene_map(c):
    return [j - (1 + 3 * c) if 1 + 3 * c <= j < 1 + 6 * c else -1 for j in range(1 + 14 * c)]


# name -> (rows, state_nuc): the gene models of 1, 2, 3 and 18 copies, the limits with an identity map, several states
# per row with entries outside 0..rows-1, and one free state
ROWMAPS = {"c1": (3, gene_map(1)), "c2": (6, gene_map(2)), "c3": (9, gene_map(3)), "c18": (54, gene_map(18)),
           "id256": (256, list(range(256))),
           "multi": (7, [0, 3, 3, -1, 6, 9, 1 << 20, -5, 2, 2] + [(5 * j) % 7 for j in range(27)] + [-1, 0, 7]),
           "q1free": (1, [-1])}


def make_nucleotides(b, L, g):
    """The nucleotide mix of test_emitter_grad_gpu.make_inputs(soft=True), plus 10 % all-zero rows (padding)."""
    nuc = torch.nn.functional.one_hot(torch.randint(0, 5, (1, b, L), generator=g), 5).float()      # one-hot with N
    kind = torch.rand((1, b, L), generator=g)
    softrows = torch.softmax(torch.randn((1, b, L, 5), generator=g), -1)
    nuc = torch.where((kind < 0.15)[..., None], softrows, nuc)                                  # genuinely soft rows
    nuc[..., 4] = torch.where((kind >= 0.15) & (kind < 0.2), torch.full_like(kind, 0.5), nuc[..., 4])   # N flag != 1
    both = (kind >= 0.2) & (kind < 0.25)
    nuc[..., 4] = torch.where(both, torch.ones_like(kind), nuc[..., 4])                         # N == 1 next to a base
    nuc = torch.where((kind >= 0.9)[..., None], torch.zeros_like(nuc), nuc)                     # padding
    return nuc


def factor(nuc, P, state_nuc):
    """The factor in the dtype of its arguments: (b, L, 5), (rows, 4), list -> (b, L, q)."""
    rows = P.shape[0]
    acgt = nuc[..., :4] + nuc[..., 4:] / 4
    idx = torch.tensor([min(max(r, 0), rows - 1) for r in state_nuc])
    free = torch.tensor([r < 0 for r in state_nuc])
    f = acgt @ P[idx].T
    return torch.where(free, torch.full_like(f, 0.25), f)


@functools.lru_cache(maxsize=None)
def reference(b, L, rowmap):
    """One (shape, row map): inputs, the fp64 factor, and the gradients of loss = (E_in f dE).sum() for P in fp64 and
    through the same torch ops in fp32 (CPU).  Computed once, shared, never modified."""
    rows, state_nuc = ROWMAPS[rowmap]
    q = len(state_nuc)
    g = torch.Generator().manual_seed(1000 * b + 7 * L + 13 * q + rows)
    nuc = make_nucleotides(b, L, g)[0]
    P = torch.softmax(torch.randn((rows, 4), generator=g), -1)
    Ein = 0.5 + torch.rand((b, L, q), generator=g)
    dE = torch.randn((b, L, q), generator=g)
    f64 = factor(nuc.double(), P.double(), state_nuc)
    dP = {}
    for dtype in (torch.float64, torch.float32):
        Pv = P.to(dtype).requires_grad_(True)
        (factor(nuc.to(dtype), Pv, state_nuc) * Ein.to(dtype) * dE.to(dtype)).sum().backward()
        dP[dtype] = torch.zeros((rows, 4), dtype=torch.float64) if Pv.grad is None else Pv.grad.double()
    return dict(nuc=nuc, P=P, Ein=Ein, dE=dE, f64=f64, dP64=dP[torch.float64], dP32=dP[torch.float32],
                tab=torch.tensor(state_nuc, dtype=torch.int32), q=q, rows=rows)


def place(c, in_place):
    """x on the device and the nucleotides' first column: ld = 5, or in place at ld = 15 + 4 + 5 with NaN elsewhere."""
    if not in_place:
        return c["nuc"].to(DEV).contiguous(), 0
    b, L = c["nuc"].shape[:2]
    x = torch.full((b, L, 15 + 4 + 5), float("nan"))
    x[..., 19:] = c["nuc"]
    return x.to(DEV), 19


def check_elementwise(got, ref, tag):
    got = got.cpu().double()
    zero = ref == 0
    assert bool(torch.isfinite(got).all()), tag
    assert bool((got[zero] == 0).all()), tag
    err = float(((got - ref).abs()[~zero] / ref.abs()[~zero]).max()) if bool((~zero).any()) else 0.0
    print("%s: %d zeros, max rel err %.3g = %.3g of the bound" % (tag, int(zero.sum()), err, err / EPS))
    assert err <= EPS, (tag, err, EPS)


@pytest.mark.parametrize("b,L", SHAPES)
@pytest.mark.parametrize("rowmap", list(ROWMAPS))
def test_forward_kernel_against_fp64(rowmap, b, L):
    c = reference(b, L, rowmap)
    P, tab = c["P"].to(DEV), c["tab"].to(DEV)
    for in_place in (False, True):
        x, col0 = place(c, in_place)
        for multiply in (0, 1):
            E = c["Ein"].to(DEV).clone() if multiply else None
            out = engine.nucleotide_emissions(x, col0, P, tab, E=E)
            assert (out is E) if multiply else tuple(out.shape) == (b, L, c["q"])
            ref = c["f64"] * c["Ein"].double() if multiply else c["f64"]
            check_elementwise(out, ref, "%s (%d,%d) in_place=%d multiply=%d" % (rowmap, b, L, in_place, multiply))


@pytest.mark.parametrize("b,L", SHAPES)
@pytest.mark.parametrize("rowmap", list(ROWMAPS))
def test_backward_kernel_against_fp64(rowmap, b, L):
    c = reference(b, L, rowmap)
    P, tab = c["P"].to(DEV), c["tab"].to(DEV)
    Ein, dE = c["Ein"].to(DEV), c["dE"].to(DEV)
    for in_place in (False, True):
        x, col0 = place(c, in_place)
        dE_in, dP = engine.nucleotide_emissions_grad(x, col0, P, tab, dE, E_in=Ein)
        tag = "%s (%d,%d) in_place=%d" % (rowmap, b, L, in_place)
        check_elementwise(dE_in, c["dE"].double() * c["f64"], tag + " dE_in")
        got, ref = dP.cpu().double(), c["dP64"]
        assert tuple(got.shape) == (c["rows"], 4) and bool(torch.isfinite(got).all())
        scale = float(ref.abs().max())
        if all(r < 0 for r in ROWMAPS[rowmap][1]):          # no state reads P: its gradient is written as 0
            assert scale == 0.0 and float(got.abs().max()) == 0.0
            continue
        e32 = float((c["dP32"] - ref).abs().max())
        err = float((got - ref).abs().max())
        bound = max(4 * e32, 2e-6 * scale)
        print("%s dP: max|ref| %.4g  e32 %.3g  kernel err %.3g = %.3g of the bound" % (tag, scale, e32, err, err / bound))
        assert scale > 0
        assert err <= bound, (tag, err, bound)
        unused = torch.tensor([r not in [min(max(s, 0), c["rows"] - 1) for s in ROWMAPS[rowmap][1] if s >= 0]
                               for r in range(c["rows"])])
        assert float(got[unused].abs().max() if bool(unused.any()) else 0.0) == 0.0


@pytest.mark.parametrize("rowmap,b,L", [("c1", 5, 4099), ("c18", 2, 1100), ("multi", 4, 37), ("id256", 7, 16)])
def test_repeated_calls_and_outputs_alone_are_bit_identical(rowmap, b, L):
    c = reference(b, L, rowmap)
    P, tab = c["P"].to(DEV), c["tab"].to(DEV)
    Ein, dE = c["Ein"].to(DEV), c["dE"].to(DEV)
    x, col0 = place(c, True)
    for multiply in (0, 1):
        one = engine.nucleotide_emissions(x, col0, P, tab, E=Ein.clone() if multiply else None)
        two = engine.nucleotide_emissions(x, col0, P, tab, E=Ein.clone() if multiply else None)
        assert torch.equal(one, two)
    for E_in in (Ein, None):
        dE_in, dP = engine.nucleotide_emissions_grad(x, col0, P, tab, dE, E_in=E_in)
        dE_in2, dP2 = engine.nucleotide_emissions_grad(x, col0, P, tab, dE, E_in=E_in)
        assert torch.equal(dE_in, dE_in2) and torch.equal(dP, dP2)
        only, none = engine.nucleotide_emissions_grad(x, col0, P, tab, dE, E_in=E_in, want_dP=False)
        assert none is None and torch.equal(only, dE_in)
        none, only = engine.nucleotide_emissions_grad(x, col0, P, tab, dE, E_in=E_in, want_dE_in=False)
        assert none is None and torch.equal(only, dP)
        assert engine.nucleotide_emissions_grad(x, col0, P, tab, dE, E_in=E_in, want_dE_in=False,
                                                want_dP=False) == (None, None)
    # E_in = None is E_in = 1
    ones = engine.nucleotide_emissions_grad(x, col0, P, tab, dE, E_in=torch.ones_like(Ein))
    assert torch.equal(ones[0], dE_in) and torch.equal(ones[1], dP)


def test_graph_capture_replays_the_eager_result():
    b, L = 2, 1100
    c = reference(b, L, "c2")
    P, tab = c["P"].to(DEV), c["tab"].to(DEV)
    Ein, dE = c["Ein"].to(DEV), c["dE"].to(DEV)
    x, col0 = place(c, True)
    eager = engine.nucleotide_emissions(x, col0, P, tab, E=Ein.clone())
    eager_dE_in, eager_dP = engine.nucleotide_emissions_grad(x, col0, P, tab, dE, E_in=Ein)     # sizes the workspace
    static = Ein.clone()
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):          # one stream, no branches
            engine.nucleotide_emissions(x, col0, P, tab, E=static)
            dE_in, dP = engine.nucleotide_emissions_grad(x, col0, P, tab, dE, E_in=Ein)
    static.copy_(Ein)                                          # capture does not run the kernels; replay does
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(static, eager) and torch.equal(dE_in, eager_dE_in) and torch.equal(dP, eager_dP)


# ------------------------------------------------------------------------------------------------ module level

# name -> (emitter arguments, embedding columns)
MODELS = {"c1": (dict(), 0), "c2_shared": (dict(num_copies=2), 0),
          "c2_unshared": (dict(num_copies=2, share_intron_parameters=False), 0), "c3": (dict(num_copies=3), 0),
          "c1_d4": (dict(), 4), "c2_d4": (dict(num_copies=2), 4), "c3_d4": (dict(num_copies=3), 4)}


def make_emitter(model, g, **extra):
    kw, d = MODELS[model]
    emb = dict(emit_embeddings=True, embedding_dim=d, temperature=float(d)) if d else {}
    em = GenePredHMMEmitter(**CODONS, trainable_nucleotides_at_exons=True, **emb, **kw, **extra)
    em.build((1, 1, 1, 15))
    with torch.no_grad():
        em.emission_kernel.copy_(torch.randn(em.emission_kernel.shape, generator=g))
        em.nuc_emission_kernel.copy_(torch.randn(em.nuc_emission_kernel.shape, generator=g))
        if d:
            ker = torch.randn(em.embedding_emission_kernel.shape, generator=g)
            ker[..., d:] = 0.3 + 0.3 * ker[..., d:]
            em.embedding_emission_kernel.copy_(ker)
    return em, d


def make_inputs(b, L, d, g):
    parts = [torch.softmax(2 * torch.randn((1, b, L, 15), generator=g), -1)]
    if d:
        parts.append(torch.randn((1, b, L, d), generator=g))
    parts.append(make_nucleotides(b, L, g))
    return torch.cat(parts, -1)


@pytest.mark.parametrize("b,L", [(3, 1), (3, 2), (3, 5), (4, 37), (2, 1100)])
@pytest.mark.parametrize("model", ["c1", "c2_shared", "c3", "c1_d4", "c2_d4", "c3_d4"])
def test_forward_fused_matches_forward(model, b, L):
    """The tolerance of test_embedding_emitter_gpu.test_forward_fused_matches_forward: max(4 e32, max|log_pdf / T| 2^-24),
    the second term only with embeddings."""
    g = torch.Generator().manual_seed(50 * b + L + len(model))
    em, d = make_emitter(model, g)
    x = make_inputs(b, L, d, g)
    hints = torch.rand((1, b, 2, em.num_states), generator=g)
    em64 = copy.deepcopy(em).double()
    dev = copy.deepcopy(em).to(DEV)
    xd = x.to(DEV)
    assert dev.can_fuse(xd)
    for training in ((False, True) if not d else (False,)):
        for h in (None, hints):
            with torch.no_grad():
                em64.recurrent_init()
                ref = em64(x.double(), end_hints=None if h is None else h.double(), training=training)
                em.recurrent_init()
                c32 = em(x, end_hints=h, training=training).double()
            got = dev.forward_fused(xd, end_hints=None if h is None else h.to(DEV), training=training)
            assert got.shape == (1, b, L, em.num_states) and not got.requires_grad
            got = got.cpu().double()
            nz = ref > 0                                           # 3-mer factors and padded rows may be exactly 0
            assert bool((got[~nz] == 0).all()) and float(ref[nz].min()) >= 1e-30
            e32 = float(((c32 - ref).abs()[nz] / ref[nz]).max())
            floor = 0.0
            if d:
                floor = float((em64.embedding_log_pdf(x.double()[0][..., 15:15 + d]) / d).detach().abs().max()) * 2.0 ** -24
            bound = max(4 * e32, floor)
            err = float(((got - ref).abs()[nz] / ref[nz]).max())
            print("%s (%d,%d) training=%s hints=%s: e32 %.3g  fused err %.3g  bound %.3g"
                  % (model, b, L, training, h is not None, e32, err, bound))
            assert err <= bound, (err, bound)
    if d:           # training=True with embeddings: the 1e-10 on the class term is not the class kernel's to add — forward()
        with torch.no_grad():
            dev.recurrent_init()
            assert torch.equal(dev.forward_fused(xd, training=True), dev(xd, training=True))


def torch_grads(em, x, G, training):
    x = x.clone().requires_grad_(True)
    em.zero_grad()
    em.recurrent_init()
    (em(x, training=training) * G).sum().backward()
    out = {n: p.grad.detach().clone().double() for n, p in em.named_parameters()}
    out["x"] = x.grad.detach().double()
    return out


@pytest.mark.parametrize("b,L", [(3, 5), (4, 37), (2, 1100)])
@pytest.mark.parametrize("model", ["c1", "c2_shared", "c2_unshared", "c3", "c1_d4", "c2_d4"])
def test_forward_fused_trainable_against_fp64_autograd(model, b, L):
    g = torch.Generator().manual_seed(1000 * b + L + len(model))
    em, d = make_emitter(model, g)
    x = make_inputs(b, L, d, g)
    G = torch.randn((1, b, L, em.num_states), generator=g)
    for training in (True, False):
        ref = torch_grads(copy.deepcopy(em).double(), x.double(), G.double(), training)
        c32 = torch_grads(copy.deepcopy(em), x, G, training)
        dev = copy.deepcopy(em).to(DEV)
        xd = x.to(DEV).requires_grad_(True)
        assert dev.can_fuse(xd)
        E = dev.forward_fused_trainable(xd, training=training)
        (E * G.to(DEV)).sum().backward()
        torch.cuda.synchronize()
        got = {n: p.grad.detach().cpu().double() for n, p in dev.named_parameters()}
        got["x"] = xd.grad.detach().cpu().double()
        names = ["x", "emission_kernel", "nuc_emission_kernel"] + (["embedding_emission_kernel"] if d else [])
        for n in names:
            a, r, c = got[n], ref[n], c32[n]
            if n == "x":                                      # the class columns
                a, r, c = a[..., :15], r[..., :15], c[..., :15]
            scale = float(r.abs().max())
            e32 = float((c - r).abs().max())
            err = float((a - r).abs().max())
            bound = max(4 * e32, 2e-6 * scale)
            print("%s (%d,%d) training=%s %s: max|ref| %.4g  e32 %.3g  err %.3g  bound %.3g"
                  % (model, b, L, training, n, scale, e32, err, bound))
            assert scale > 0
            assert err <= bound, (n, err, bound)
        assert float(got["x"][..., -5:].abs().max()) == 0.0    # nucleotides are data: exactly 0


# ------------------------------------------------------------------------------------------------ layer level

def gene_cell(model, b, L, seed):
    g = torch.Generator().manual_seed(seed)
    em, d = make_emitter(model, g, fused_training=True)
    cls = torch.softmax(2 * torch.randn((1, b, L, 15), generator=g), -1)
    parts = [cls] + ([torch.randn((1, b, L, d), generator=g)] if d else [])
    parts.append(torch.nn.functional.one_hot(torch.randint(0, 5, (1, b, L), generator=g), 5).float())
    copies = em.num_copies
    kw = dict(k=copies) if copies > 1 else {}
    tr = GenePredMultiHMMTransitioner(initial_exon_len=200, initial_intron_len=4500, initial_ir_len=10000, **kw)
    return HmmCell([em.num_states], 15, em, tr), torch.cat(parts, -1)


@pytest.mark.parametrize("model", ["c1", "c2_d4"])
def test_layer_inference_through_the_fused_path(model, monkeypatch):
    """Tolerances of test_embedding_emitter_gpu.test_layer_inference_through_the_fused_path."""
    b, L = 3, 450
    cell, x = gene_cell(model, b, L, 21)
    cell, x = cell.to(DEV), x.to(DEV)
    em = cell.emitter[0]
    assert em.fused_training and em.can_fuse(x)
    layer = MsaHmmLayer(cell, use_prior=False)
    layer.build(x.shape)
    calls = []
    real = engine.nucleotide_emissions
    monkeypatch.setattr(engine, "nucleotide_emissions", lambda *a, **k: (calls.append(1), real(*a, **k))[1])

    def run():
        with torch.no_grad():
            post = layer.state_posterior_log_probs(x)
            path, score = Viterbi.viterbi(x, cell)
            loglik, mean = layer(x)
        return post, path, score, loglik

    post, path, score, loglik = run()
    assert len(calls) == 3                                     # every call went through the kernel
    monkeypatch.setattr(em, "can_fuse", lambda inputs: False)  # the same calls through forward()
    post_t, path_t, score_t, loglik_t = run()
    assert len(calls) == 3
    q = em.num_states
    assert post.shape == (1, b, L, q) and path.shape == (1, b, L)
    assert float((post.exp() - post_t.exp()).abs().max()) <= 2e-5
    assert float((post.exp().sum(-1) - 1).abs().max()) <= 2e-5
    assert bool(((loglik - loglik_t).abs() <= 1e-6 * loglik_t.abs() + 2e-4).all())
    assert bool(((score - score_t).abs() <= 1e-6 * score_t.abs() + 2e-4).all())
    assert float((path != path_t).float().mean()) <= 0.01


@pytest.mark.parametrize("model", ["c1", "c2_d4"])
def test_layer_trains_the_nucleotide_kernel(model):
    """One training step on the log-likelihood against fp64 CPU autograd through an fp64 copy of the module and the
    oracle's log-likelihood; the layer tolerance of test_emitter_grad_gpu: 5e-4 scale + 1e-7."""
    b, L = 3, 60
    cell, x = gene_cell(model, b, L, 33)
    cpu = gene_cell(model, b, L, 33)[0].double()              # same seed: identical parameters
    cell, xd = cell.to(DEV), x.to(DEV)
    assert cell.emitter[0].can_fuse(xd)
    layer = MsaHmmLayer(cell, use_prior=False)
    layer.build(xd.shape)
    loglik, mean = layer(xd, training=True)
    (-mean).backward()
    torch.cuda.synchronize()
    got = {n: p.grad.detach().cpu().double() for n, p in cell.named_parameters() if p.grad is not None}
    name = "emitter.0.nuc_emission_kernel"
    assert name in got, sorted(got)

    cpu.recurrent_init()
    E = cpu.emission_probs(x.double(), end_hints=None, training=True)[0]
    _, ll = torch64.posterior(cpu.A[0], cpu.init_dist.reshape(-1), E, eps=cpu.epsilon)
    (-ll.mean()).backward()
    assert bool(((loglik[0].cpu().double() - ll.detach()).abs() <= 1e-6 * ll.detach().abs() + 2e-3).all())
    for n in (name, "emitter.0.emission_kernel"):
        want = dict(cpu.named_parameters())[n].grad
        scale = float(want.abs().max())
        err = float((got[n] - want).abs().max())
        print("%s %s: scale %.4g err %.3g" % (model, n, scale, err))
        assert bool(torch.isfinite(got[n]).all()) and float(got[n].abs().max()) > 0
        assert err <= 5e-4 * scale + 1e-7, (n, err, scale)
