"""hmm_embedding_emissions on a HIP device: the kernel against an fp64 restatement of the density, its
determinism and graph capture, and the layer (posteriors, Viterbi, likelihood, one training step) with an
embedding emitter.  Needs an MI355X.

Tolerance of the kernel tests: per case the fp32 torch path (SimpleGenePredHMMEmitter.embedding_log_pdf, exp,
the product with E) is run on the CPU too; e32 is its maximum relative error against fp64.  The kernel must
satisfy max rel err <= max(4 e32, max|log_pdf / T| 2^-24): the factor 4 covers another summation order over d,
nothing else; the second term is the rounding of exp's fp32 argument itself, a floor under any fp32 evaluation
(it takes over only where the CPU path happens to round luckily on a small case).  Every element is compared:
each case first asserts that its fp64 reference is >= 1e-30 everywhere."""
import copy
import functools
import math

import pytest
import torch

from hmm_layer_amd import Viterbi, engine
from hmm_layer_amd.MsaHmmCell import HmmCell
from hmm_layer_amd.MsaHMMLayer import MsaHmmLayer
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
ROWMAPS = {"r5": (5, list(range(5))), "r13": (13, list(range(13))), "r16": (16, list(range(16))),
           "r17": (17, list(range(17))), "r32": (32, list(range(32))),
           "q15": (13, [0, 1, 1, 1] + list(range(2, 13))),
           "q29": (25, [0, 1, 2, 1, 2, 1, 2] + list(range(3, 25)))}


def shell(d, ker):
    """An emitter object carrying a (rows, 2d) parameter: rows need not be a model's row count here."""
    em = SimpleGenePredHMMEmitter(emit_embeddings=True, embedding_dim=d)
    em.embedding_emission_kernel = torch.nn.Parameter(ker.reshape(1, ker.shape[0], 1, 2 * d).clone())
    return em


@functools.lru_cache(maxsize=None)
def reference(b, L, d, rowmap, far):
    """One (shape, d, rows, input kind): parameter, inputs, fp64 log_pdf and the fp32 torch path's log_pdf (CPU)."""
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
    return dict(em=em, emb=emb, lp64=lp64, lp32=lp32, Ein=Ein, row=torch.tensor(state_row, dtype=torch.int32))


def run_kernel(c, d, s, T, add, multiply):
    """The kernel on an (b, L, s + d + 5) tensor whose other columns are NaN -> E on the CPU, fp64."""
    b, L = c["emb"].shape[:2]
    x = torch.full((b, L, s + d + 5), float("nan"))
    x[..., s:s + d] = c["emb"]
    mean, inv_std, log_norm = c["em"].embedding_tables(torch.device(DEV))
    E = c["Ein"].to(DEV).clone() if multiply else None
    out = engine.embedding_emissions(x.to(DEV), s, d, mean, inv_std, log_norm, c["row"].to(DEV), E=E,
                                     inv_temperature=1.0 / T, add=add)
    assert (out is E) if multiply else tuple(out.shape) == (b, L, c["row"].numel())
    return out.cpu().double()


@pytest.mark.parametrize("b,L", SHAPES)
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("rowmap", list(ROWMAPS))
def test_kernel_against_fp64(rowmap, d, b, L):
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
                        got = run_kernel(c, d, s, T, add, multiply)
                        assert bool(torch.isfinite(got).all())
                        err = float(((got - ref).abs() / ref).max())
                        worst = max(worst, err / bound)
                        print("%s d=%d (%d,%d) far=%d T=%g add=%g mult=%d s=%d: min ref %.3g  e32 %.3g  floor %.3g  "
                              "kernel err %.3g" % (rowmap, d, b, L, far, T, add, multiply, s, float(ref.min()), e32,
                                                   floor, err))
                        assert err <= bound, (far, T, add, multiply, s, err, bound)
    print("worst err / bound %.3g" % worst)


@pytest.mark.parametrize("rowmap,d,b,L", [("q15", 64, 2, 1100), ("r32", 130, 4, 37), ("q29", 17, 7, 16)])
def test_repeated_calls_are_bit_identical(rowmap, d, b, L):
    c = reference(b, L, d, rowmap, False)
    for multiply in (0, 1):
        one = run_kernel(c, d, 15, float(d), 0.0, multiply)
        two = run_kernel(c, d, 15, float(d), 0.0, multiply)
        assert torch.equal(one, two)


def test_graph_capture_replays_the_eager_result():
    b, L, d, s = 2, 1100, 64, 15
    c = reference(b, L, d, "q15", False)
    x = torch.full((b, L, s + d + 5), float("nan"))
    x[..., s:s + d] = c["emb"]
    x = x.to(DEV)
    mean, inv_std, log_norm = c["em"].embedding_tables(torch.device(DEV))
    row = c["row"].to(DEV)
    eager = engine.embedding_emissions(x, s, d, mean, inv_std, log_norm, row, E=c["Ein"].to(DEV).clone(),
                                       inv_temperature=1.0 / d)
    static = c["Ein"].to(DEV).clone()
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):          # one stream, no branches
            engine.embedding_emissions(x, s, d, mean, inv_std, log_norm, row, E=static, inv_temperature=1.0 / d)
    static.copy_(c["Ein"])                                     # capture does not run the kernel; replay does
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(static, eager)


# ------------------------------------------------------------------------------------------------ layer level

def make_inputs(b, L, s, d, soft, g):
    """The input mix of test_emitter_grad_gpu.make_inputs with d embedding columns between classes and nucleotides."""
    cls = torch.softmax(2 * torch.randn((1, b, L, s), generator=g), -1)
    emb = torch.randn((1, b, L, d), generator=g)
    nuc = torch.nn.functional.one_hot(torch.randint(0, 5, (1, b, L), generator=g), 5).float()      # one-hot with N
    if soft:
        kind = torch.rand((1, b, L), generator=g)
        softrows = torch.softmax(torch.randn((1, b, L, 5), generator=g), -1)
        nuc = torch.where((kind < 0.15)[..., None], softrows, nuc)                                  # genuinely soft rows
        nuc[..., 4] = torch.where((kind >= 0.15) & (kind < 0.2), torch.full_like(kind, 0.5), nuc[..., 4])   # N flag != 1
        both = (kind >= 0.2) & (kind < 0.25)
        nuc[..., 4] = torch.where(both, torch.ones_like(kind), nuc[..., 4])                         # N == 1 next to a base
    return torch.cat([cls, emb, nuc], -1)


MODELS = {"q15_d16": (1, 16), "q29_d5": (2, 5)}             # name -> (copies, d)


def make_emitter(model, g):
    copies, d = MODELS[model]
    em = GenePredHMMEmitter(**CODONS, num_copies=copies, emit_embeddings=True, embedding_dim=d, temperature=float(d))
    em.build((1, 1, 1, 15))
    with torch.no_grad():
        em.emission_kernel.copy_(torch.randn(em.emission_kernel.shape, generator=g))
        ker = torch.randn(em.embedding_emission_kernel.shape, generator=g)
        ker[..., d:] = 0.3 + 0.3 * ker[..., d:]
        em.embedding_emission_kernel.copy_(ker)
    return em, d


@pytest.mark.parametrize("b,L", [(3, 5), (4, 37), (2, 1100)])
@pytest.mark.parametrize("model", list(MODELS))
def test_forward_fused_matches_forward(model, b, L):
    g = torch.Generator().manual_seed(50 * b + L + len(model))
    em, d = make_emitter(model, g)
    x = make_inputs(b, L, 15, d, True, g)
    hints = torch.rand((1, b, 2, em.num_states), generator=g)
    em64 = copy.deepcopy(em).double()
    dev = copy.deepcopy(em).to(DEV)
    xd = x.to(DEV)
    assert dev.can_fuse(xd)
    for h in (None, hints):
        with torch.no_grad():
            em64.recurrent_init()
            ref = em64(x.double(), end_hints=None if h is None else h.double())
            em.recurrent_init()
            c32 = em(x, end_hints=h).double()
            dev.recurrent_init()
            want = dev(xd, end_hints=None if h is None else h.to(DEV)).cpu().double()
        got = dev.forward_fused(xd, end_hints=None if h is None else h.to(DEV))
        assert got.shape == (1, b, L, em.num_states) and not got.requires_grad
        got = got.cpu().double()
        nz = ref > 0                                           # 3-mer factors may be exactly 0, in every path
        assert bool((got[~nz] == 0).all()) and float(ref[nz].min()) >= 1e-30
        e32 = float(((c32 - ref).abs()[nz] / ref[nz]).max())
        lp = em64.embedding_log_pdf(x.double()[0][..., 15:15 + d]) / d
        bound = max(4 * e32, float(lp.abs().max()) * 2.0 ** -24)
        err = float(((got - ref).abs()[nz] / ref[nz]).max())
        dev_err = float(((want - ref).abs()[nz] / ref[nz]).max())
        print("%s (%d,%d) hints=%s: e32 %.3g  fused err %.3g  device forward() err %.3g  bound %.3g"
              % (model, b, L, h is not None, e32, err, dev_err, bound))
        assert err <= bound, (err, bound)
    # training=True: the 1e-10 on the class term is not the class kernel's to add — forward()
    with torch.no_grad():
        dev.recurrent_init()
        assert torch.equal(dev.forward_fused(xd, training=True), dev(xd, training=True))


def gene_cell(model, b, L, seed):
    g = torch.Generator().manual_seed(seed)
    em, d = make_emitter(model, g)
    x = make_inputs(b, L, 15, d, False, g)
    copies = MODELS[model][0]
    kw = dict(k=copies) if copies > 1 else {}
    tr = GenePredMultiHMMTransitioner(initial_exon_len=200, initial_intron_len=4500, initial_ir_len=10000, **kw)
    return HmmCell([em.num_states], 15, em, tr), x


@pytest.mark.parametrize("model", list(MODELS))
def test_layer_inference_through_the_fused_path(model, monkeypatch):
    b, L = 3, 450
    cell, x = gene_cell(model, b, L, 21)
    cell, x = cell.to(DEV), x.to(DEV)
    em = cell.emitter[0]
    layer = MsaHmmLayer(cell, use_prior=False)
    layer.build(x.shape)
    calls = []
    real = engine.embedding_emissions
    monkeypatch.setattr(engine, "embedding_emissions", lambda *a, **k: (calls.append(1), real(*a, **k))[1])

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


@pytest.mark.parametrize("model", list(MODELS))
def test_layer_trains_the_embedding_kernel(model):
    """One training step through MsaHmmLayer.forward against fp64 CPU autograd through an fp64 copy of the module
    and the oracle's log-likelihood; tolerance of test_emitter_grad_gpu's layer test: 5e-4 scale + 1e-7."""
    b, L = 3, 60
    cell, x = gene_cell(model, b, L, 33)
    cpu = gene_cell(model, b, L, 33)[0].double()              # same seed: identical parameters
    cell, xd = cell.to(DEV), x.to(DEV)
    layer = MsaHmmLayer(cell, use_prior=False)
    layer.build(xd.shape)
    loglik, mean = layer(xd, training=True)
    (-mean).backward()
    torch.cuda.synchronize()
    got = {n: p.grad.detach().cpu().double() for n, p in cell.named_parameters() if p.grad is not None}
    name = "emitter.0.embedding_emission_kernel"
    assert name in got, sorted(got)

    cpu.recurrent_init()
    E = cpu.emission_probs(x.double(), end_hints=None, training=True)[0]
    A = cpu.A[0]
    pi = cpu.init_dist.reshape(-1)
    _, ll = torch64.posterior(A, pi, E, eps=cpu.epsilon)
    (-ll.mean()).backward()
    assert bool(((loglik[0].cpu().double() - ll.detach()).abs() <= 1e-6 * ll.detach().abs() + 2e-3).all())
    for n in (name, "emitter.0.emission_kernel"):
        want = dict(cpu.named_parameters())[n].grad
        scale = float(want.abs().max())
        err = float((got[n] - want).abs().max())
        print("%s %s: scale %.4g err %.3g" % (model, n, scale, err))
        assert bool(torch.isfinite(got[n]).all()) and float(got[n].abs().max()) > 0
        assert err <= 5e-4 * scale + 1e-7, (n, err, scale)
