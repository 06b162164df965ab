"""hmm_gene_emissions_wide / hmm_gene_emissions_grad_wide on a HIP device: the gene models of three to eighteen
copies (43 .. 253 states) through the fused emitter.  Needs an MI355X.

Forward: against GenePredHMMEmitter.forward in torch ops on the device (relative 2e-5) and the oracle's CPU
restatement (<= 1e-6 max|cpu|), the tolerances of test_layer_gpu.test_fused_emitter_matches_torch_emitter; direct
engine calls with synthetic tables against an fp64 restatement; bit-identity with hmm_gene_emissions where both
apply.  Backward: the method and tolerance of test_emitter_grad_gpu: fp64 CPU autograd through forward() is the
reference, e32 the error of the fp32 CPU torch path, max|got - ref| <= max(4 e32, 2e-6 max|ref|) for the class
columns of dx and for d emission_kernel; nucleotide columns of dx exactly 0.  Then graph capture and the layer
(posteriors, Viterbi, likelihood, one training step) for three and five copies."""
import copy
import functools

import numpy as np
import pytest
import torch

from hmm_layer_amd import Viterbi, engine, kmer
from hmm_layer_amd.MsaHmmCell import HmmCell
from hmm_layer_amd.MsaHMMLayer import MsaHmmLayer
from hmm_layer_amd.gene_pred_hmm_emitter import GenePredHMMEmitter
from hmm_layer_amd.gene_pred_hmm_transitioner import GenePredMultiHMMTransitioner
from oracle import params

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CODONS = dict(start_codons=[("ATG", 1.)], stop_codons=[("TAG", .34), ("TAA", .33), ("TGA", .33)],
              intron_begin_pattern=[("NGT", .99), ("NGC", .005), ("NAT", .005)],
              intron_end_pattern=[("AGN", .99), ("ACN", .01)])
# shorter than a tile, exactly one tile, a ragged tail, more than one run
SHAPES = [(3, 5), (7, 16), (4, 37), (2, 1100)]
# name -> (emitter arguments, training flag of the backward case).  q <= 64 with rows > 32 (43 / 37, 57 / 57); a
# second group of 7 states (71); one state short of two groups (127); the limit (253 states and rows)
MODELS = {
    "c3_shared": (dict(num_copies=3), True),
    "c4_unshared": (dict(num_copies=4, share_intron_parameters=False), False),
    "c5_shared": (dict(num_copies=5), True),
    "c9_shared_n_mass_compat": (dict(num_copies=9, n_mass_compat=True), True),
    "c18_unshared": (dict(num_copies=18, share_intron_parameters=False), True),
}
S = 15


def make_inputs(b, L, s, soft, g):
    cls = torch.softmax(2 * torch.randn((1, b, L, s), generator=g), -1)
    nuc = torch.nn.functional.one_hot(torch.randint(0, 5, (1, b, L), generator=g), 5).float()      # one-hot with N
    if soft:        # the mixture of test_layer_gpu.test_fused_emitter_soft_nucleotides_and_short_sequences
        kind = torch.rand((1, b, L), generator=g)
        softrows = torch.softmax(torch.randn((1, b, L, 5), generator=g), -1)
        nuc = torch.where((kind < 0.15)[..., None], softrows, nuc)                                  # genuinely soft rows
        nuc[..., 4] = torch.where((kind >= 0.15) & (kind < 0.2), torch.full_like(kind, 0.5), nuc[..., 4])   # N flag != 1
        both = (kind >= 0.2) & (kind < 0.25)
        nuc[..., 4] = torch.where(both, torch.ones_like(kind), nuc[..., 4])                         # N == 1 next to a base
    return torch.cat([cls, nuc], -1)


def make_emitter(model, b, L, g, **more):
    em = GenePredHMMEmitter(**CODONS, **MODELS[model][0], **more)
    em.build((1, b, L, S))
    with torch.no_grad():
        em.emission_kernel.copy_(torch.randn(em.emission_kernel.shape, generator=g))
    return em


# ------------------------------------------------------------------------------------------------ forward

def check_forward(em, x, cpu_oracle=None):
    dev = copy.deepcopy(em).to(DEV)
    dev.recurrent_init()
    xd = x.to(DEV)
    assert dev.can_fuse(xd) and dev.fused_route() == "wide"
    for training in (False, True):
        with torch.no_grad():
            want = dev(xd, training=training)
        got = dev.forward_fused(xd, training=training)
        assert got.shape == want.shape == (1, x.shape[1], x.shape[2], em.num_states)
        rel = float(((got - want).abs() / (want.abs() + 1e-30)).max())
        print("training=%s: max rel err against the device torch path %.3g" % (training, rel))
        assert rel < 2e-5
        if cpu_oracle is not None:
            cpu = cpu_oracle(training).numpy()
            err = float(np.abs(got.cpu().numpy() - cpu).max())
            print("training=%s: max abs err against the CPU oracle %.3g, bound %.3g" % (training, err, 1e-6 * np.abs(cpu).max()))
            assert err <= 1e-6 * np.abs(cpu).max()


@pytest.mark.parametrize("b,L", SHAPES)
@pytest.mark.parametrize("model", list(MODELS))
def test_forward_matches_torch_emitter_and_oracle(model, b, L):
    g = torch.Generator().manual_seed(100 * b + L)
    x = make_inputs(b, L, S, False, g)
    em = make_emitter(model, b, L, g)
    tab = params.codon_table(**params.DEFAULT_CODONS)
    check_forward(em, x, lambda training: params.gene_emissions(
        x, em.emission_kernel.detach(), tab, copies=em.num_copies, share_intron=em.share_intron_parameters,
        training=training, d5_compat=em.n_mass_compat))


@pytest.mark.parametrize("b,L", [(4, 37), (2, 1100)])
def test_forward_soft_nucleotides(b, L):
    """The generic path (soft rows, N flags that are not exactly 1, N next to a base) on the 71-state model."""
    g = torch.Generator().manual_seed(100 * b + L + 1)
    check_forward(make_emitter("c5_shared", b, L, g), make_inputs(b, L, S, True, g))


def synthetic(q, s, g, rows=256, nc=9, b=3, L=150):
    x = make_inputs(b, L, s, False, g)[0]
    B = torch.softmax(torch.randn((rows, s), generator=g), -1)
    row = torch.randint(0, rows, (q,), generator=g, dtype=torch.int32)
    codon = torch.rand((2, nc, 64), generator=g) * (torch.rand((2, nc, 64), generator=g) < 0.5)
    cod = torch.randint(-1, nc, (q,), generator=g, dtype=torch.int32)
    return x, B, row, codon, cod


def restatement(x, B, row, codon, cod, free_value, add, n_mass):
    """The kernel's definition (include/hmm_engine.h) in fp64 torch ops."""
    x, B, codon = x.double(), B.double(), codon.double()
    s = B.shape[1]
    emit = x[..., :s] @ B[row.long()].T
    nuc = x[..., s:]
    left = kmer.make_k_mers(nuc, 3, True).reshape(*nuc.shape[:2], 64)
    right = kmer.make_k_mers(nuc, 3, False, n_mass=n_mass).reshape(*nuc.shape[:2], 64)
    c = cod.long().clamp(min=0)
    factor = (left @ codon[0][c].T) * (right @ codon[1][c].T)
    factor = torch.where(cod >= 0, factor, torch.full_like(factor, free_value))
    return emit * (factor + add)


@pytest.mark.parametrize("s", [7, 16, 20, 32])
@pytest.mark.parametrize("q", [64, 128, 256])
def test_direct_call_with_synthetic_tables(q, s):
    """q a whole number of groups, rows = 256, random state_row and state_codon.  Tolerance: every term is
    non-negative, so the fp32 result's relative error is bounded by the number of roundings: s for the class sum,
    64 for each of the two table entries, a few products: (s + 132) 2^-24 <= 9.8e-6 < 2e-5, the project's bound."""
    g = torch.Generator().manual_seed(1000 * q + s)
    args = synthetic(q, s, g)
    for add, n_mass in ((0.0, 1), (1e-7, 2)):
        want = restatement(*args, 1.0 / 4096.0, add, n_mass)
        got = engine.gene_emissions_wide(*[a.to(DEV) for a in args], add=add, n_mass=n_mass).cpu().double()
        assert got.shape == want.shape == (3, 150, q)
        rel = float(((got - want).abs() / (want.abs() + 1e-30)).max())
        print("q %d s %d add %g: max rel err %.3g" % (q, s, add, rel))
        assert rel < 2e-5


def test_state_row_out_of_range_is_clamped():
    g = torch.Generator().manual_seed(5)
    x, B, row, codon, cod = synthetic(100, 15, g, rows=40)
    bad_row = row.clone()
    bad_row[3], bad_row[70], bad_row[99] = -7, 40, 1 << 20
    row[3], row[70], row[99] = 0, 39, 39
    dE = torch.randn((3, 150, 100), generator=g)
    a = [t.to(DEV) for t in (x, B, row, codon, cod)]
    bad = [t.to(DEV) for t in (x, B, bad_row, codon, cod)]
    assert torch.equal(engine.gene_emissions_wide(*a), engine.gene_emissions_wide(*bad))
    for u, v in zip(engine.gene_emissions_grad_wide(*a, dE.to(DEV)), engine.gene_emissions_grad_wide(*bad, dE.to(DEV))):
        assert torch.equal(u, v)


@pytest.mark.parametrize("b,L", [(4, 37), (2, 1100)])
def test_wide_forward_equals_the_64_state_forward_bit_for_bit(b, L):
    """29 states: both kernels run the same class-sum chain (<NT = 4, KT = 2>) and the same scale."""
    g = torch.Generator().manual_seed(17 * b + L)
    em = GenePredHMMEmitter(**CODONS, num_copies=2)
    em.build((1, b, L, S))
    with torch.no_grad():
        em.emission_kernel.copy_(torch.randn(em.emission_kernel.shape, generator=g))
        Bm = em.make_B()[0].to(DEV).contiguous()
    row, cod = em.state_tables(torch.device(DEV))
    codon = em.codon_probs.to(DEV, torch.float32).contiguous()
    for soft in (False, True):
        x = make_inputs(b, L, S, soft, g)[0].to(DEV)
        for add in (0.0, 1e-7):
            assert torch.equal(engine.gene_emissions_wide(x, Bm, row, codon, cod, add=add),
                               engine.gene_emissions(x, Bm, row, codon, cod, add=add))


# ------------------------------------------------------------------------------------------------ backward

@pytest.mark.parametrize("b,L", [(4, 37), (2, 1100)])
def test_wide_backward_dx_equals_the_64_state_backward_bit_for_bit(b, L):
    """29 states: one group, so both kernels run the same chain per position (H, then H Bexp over <NT = 4, KT = 2>).
    (2, 1100) has several runs, a run border inside a sequence and a ragged last tile.  dB is not compared: the two
    kernels sum it over runs of different lengths by design."""
    g = torch.Generator().manual_seed(19 * b + L)
    em = GenePredHMMEmitter(**CODONS, num_copies=2)
    em.build((1, b, L, S))
    with torch.no_grad():
        em.emission_kernel.copy_(torch.randn(em.emission_kernel.shape, generator=g))
        Bm = em.make_B()[0].to(DEV).contiguous()
    row, cod = em.state_tables(torch.device(DEV))
    codon = em.codon_probs.to(DEV, torch.float32).contiguous()
    for soft in (False, True):
        x = make_inputs(b, L, S, soft, g)[0].to(DEV)
        dE = torch.randn((b, L, em.num_states), generator=g).to(DEV)
        for add in (0.0, 1e-7):
            for want_dB in (True, False):
                wide, _ = engine.gene_emissions_grad_wide(x, Bm, row, codon, cod, dE, add=add, want_dB=want_dB)
                narrow, _ = engine.gene_emissions_grad(x, Bm, row, codon, cod, dE, add=add, want_dB=want_dB)
                assert float(wide.abs().max()) > 0
                assert torch.equal(wide, narrow), (soft, add, want_dB)


def torch_grads(em, x, G, training):
    """Autograd through GenePredHMMEmitter.forward with loss = (E G).sum(): (dx, d emission_kernel)."""
    x = x.clone().requires_grad_(True)
    em.zero_grad()
    em.recurrent_init()
    E = em(x, training=training)
    (E * G).sum().backward()
    return x.grad.detach(), em.emission_kernel.grad.detach().clone()


@functools.lru_cache(maxsize=None)
def case(model, b, L, soft=False):
    """One (model, shape): fp64 CPU reference, fp32 CPU error, the kernel's result.  Computed once, shared."""
    training = MODELS[model][1]
    g = torch.Generator().manual_seed(1000 * b + L + 7 * S + int(soft))
    x = make_inputs(b, L, S, soft, g)
    em = make_emitter(model, b, L, g)
    G = torch.randn((1, b, L, em.num_states), generator=g)
    ref_dx, ref_dk = torch_grads(copy.deepcopy(em).double(), x.double(), G.double(), training)
    c32_dx, c32_dk = torch_grads(copy.deepcopy(em), x, G, training)
    dev = copy.deepcopy(em).to(DEV)
    xd = x.to(DEV).requires_grad_(True)
    assert dev.can_fuse(xd) and dev.fused_route() == "wide"
    E = dev.forward_fused_trainable(xd, training=training)
    (E * G.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    return dict(ref_dx=ref_dx, ref_dk=ref_dk, c32_dx=c32_dx.double(), c32_dk=c32_dk.double(),
                got_dx=xd.grad.detach().cpu().double(), got_dk=dev.emission_kernel.grad.detach().cpu().double(),
                em=em, x=x, G=G, training=training)


def check_case(c, tag):
    s = S
    for name, got, ref, c32 in (("dx", c["got_dx"][..., :s], c["ref_dx"][..., :s], c["c32_dx"][..., :s]),
                                ("d emission_kernel", c["got_dk"], c["ref_dk"], c["c32_dk"])):
        scale = float(ref.abs().max())
        e32 = float((c32 - ref).abs().max())
        err = float((got - ref).abs().max())
        bound = max(4 * e32, 2e-6 * scale)
        print("%s %s: max|ref| %.4g  e32 %.3g (%.3g rel)  kernel err %.3g (%.3g rel)  bound %.3g"
              % (tag, name, scale, e32, e32 / scale, err, err / scale, bound))
        assert scale > 0
        assert err <= bound, (tag, name, err, bound)
    assert float(c["got_dx"][..., s:].abs().max()) == 0.0          # nucleotide columns: exactly 0


@pytest.mark.parametrize("b,L", SHAPES)
@pytest.mark.parametrize("model", list(MODELS))
def test_backward_against_fp64_autograd(model, b, L):
    check_case(case(model, b, L), "%s (%d, %d)" % (model, b, L))


def test_backward_several_runs_per_sequence():
    check_case(case("c5_shared", 5, 4099), "c5_shared (5, 4099)")


@pytest.mark.parametrize("b,L", [(4, 37), (2, 1100)])
def test_backward_soft_nucleotides(b, L):
    check_case(case("c5_shared", b, L, True), "c5_shared soft (%d, %d)" % (b, L))


def engine_args(c):
    em = copy.deepcopy(c["em"]).to(DEV)
    row, cod = em.state_tables(torch.device(DEV))
    with torch.no_grad():
        B = em.make_B()[0].contiguous()
    kw = dict(add=1e-7 if c["training"] else 0.0, n_mass=2 if em.n_mass_compat else 1)
    return (c["x"][0].to(DEV).contiguous(), B, row, em.codon_probs.to(DEV, torch.float32).contiguous(), cod), kw


@pytest.mark.parametrize("model,b,L", [("c5_shared", 5, 4099), ("c18_unshared", 2, 1100), ("c3_shared", 4, 37)])
def test_outputs_alone_and_repeated_are_bit_identical(model, b, L):
    c = case(model, b, L)
    args, kw = engine_args(c)
    G = c["G"][0].to(DEV).contiguous()
    dx, dB = engine.gene_emissions_grad_wide(*args, G, **kw)
    dx2, dB2 = engine.gene_emissions_grad_wide(*args, G, **kw)
    assert torch.equal(dx, dx2) and torch.equal(dB, dB2)
    only_dx, none = engine.gene_emissions_grad_wide(*args, G, want_dB=False, **kw)
    assert none is None and torch.equal(only_dx, dx)
    none, only_dB = engine.gene_emissions_grad_wide(*args, G, want_dx=False, **kw)
    assert none is None and torch.equal(only_dB, dB)
    assert engine.gene_emissions_grad_wide(*args, G, want_dx=False, want_dB=False, **kw) == (None, None)
    assert torch.equal(engine.gene_emissions_wide(*args, **kw), engine.gene_emissions_wide(*args, **kw))
    # the node's result is the direct call's
    assert torch.equal(dx.cpu().double(), c["got_dx"][0])


@pytest.mark.parametrize("model,b,L,at", [("c5_shared", 2, 1100, (0, 1023)), ("c5_shared", 2, 1100, (1, 0)),
                                          ("c18_unshared", 4, 37, (2, 36)), ("c3_shared", 7, 16, (3, 15))])
def test_gradient_at_one_position_stays_there(model, b, L, at):
    c = case(model, b, L)
    args, kw = engine_args(c)
    G = torch.zeros_like(c["G"][0])
    G[at] = c["G"][0][at]
    dx, dB = engine.gene_emissions_grad_wide(*args, G.to(DEV), **kw)
    nz = dx.abs().sum(-1).cpu()
    assert float(nz[at]) > 0
    nz[at] = 0
    assert float(nz.max()) == 0.0
    assert bool(torch.isfinite(dB).all()) and float(dB.abs().max()) > 0


def test_graph_capture_and_replay():
    """Forward and backward of the 71-state model captured on one stream (a single chain, no branches), replayed
    once: bit-identical to the eager calls."""
    c = case("c5_shared", 2, 1100)
    args, kw = engine_args(c)
    G = c["G"][0].to(DEV).contiguous()
    eager = (engine.gene_emissions_wide(*args, **kw),) + engine.gene_emissions_grad_wide(*args, G, **kw)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):          # one stream, no branches
            static = (engine.gene_emissions_wide(*args, **kw),) + engine.gene_emissions_grad_wide(*args, G, **kw)
    for t in static:
        t.fill_(float("nan"))                                  # capture does not run the kernels; replay does
    graph.replay()
    torch.cuda.synchronize()
    for n, a, e in zip(("E", "dx", "dB"), static, eager):
        assert torch.equal(a, e), n


# ------------------------------------------------------------------------------------------------ layer level

def gene_cell(copies, b, L, seed, fused_training=False):
    g = torch.Generator().manual_seed(seed)
    x = make_inputs(b, L, S, False, g)
    em = GenePredHMMEmitter(**CODONS, num_copies=copies, fused_training=fused_training)
    em.build((1, b, L, S))
    with torch.no_grad():
        em.emission_kernel.copy_(torch.randn(em.emission_kernel.shape, generator=g))
    tr = GenePredMultiHMMTransitioner(k=copies, initial_exon_len=200, initial_intron_len=4500, initial_ir_len=10000)
    return HmmCell([em.num_states], S, em, tr).to(DEV), x.to(DEV)


def count_calls(monkeypatch, name):
    calls = []
    real = getattr(engine, name)
    monkeypatch.setattr(engine, name, lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    return calls


@pytest.mark.parametrize("copies", [3, 5])
def test_layer_inference_through_the_wide_kernel(copies, monkeypatch):
    """Posteriors, Viterbi and the likelihood of the 43- and 71-state models: the fused path (which raised
    EngineError for three copies and was not taken for five before hmm_gene_emissions_wide) against forward()."""
    b, L = 3, 200
    cell, x = gene_cell(copies, b, L, 21)
    em = cell.emitter[0]
    layer = MsaHmmLayer(cell, use_prior=False)
    layer.build(x.shape)
    calls = count_calls(monkeypatch, "gene_emissions_wide")

    def run():
        with torch.no_grad():
            post = layer.state_posterior_log_probs(x)
            path, score = Viterbi.viterbi(x, cell)
            loglik, mean = layer(x)
        return post, path, score, loglik

    post, path, score, loglik = run()
    assert len(calls) == 3                                     # every call went through the wide kernel
    monkeypatch.setattr(em, "can_fuse", lambda inputs: False)  # the same calls through forward()
    post_t, path_t, score_t, loglik_t = run()
    assert len(calls) == 3
    q = em.num_states
    assert q == 1 + 14 * copies and post.shape == (1, b, L, q) and path.shape == (1, b, L)
    # tolerances of test_embedding_emitter_gpu.test_layer_inference_through_the_fused_path
    assert float((post.exp() - post_t.exp()).abs().max()) <= 2e-5
    assert float((post.exp().sum(-1) - 1).abs().max()) <= 2e-5
    assert bool(((loglik - loglik_t).abs() <= 1e-6 * loglik_t.abs() + 2e-4).all())
    # Viterbi: the two E tensors differ in their last bits, so the best scores agree to 1e-4 (relative: a score is a
    # sum of L logs), and a sequence's two paths differ only where that difference decides a near-tie
    print("viterbi scores", score.flatten().tolist(), score_t.flatten().tolist(),
          "paths differ at %d positions" % int((path != path_t).sum()))
    assert bool(((score - score_t).abs() <= 1e-4 * score_t.abs().clamp(min=1.0)).all())
    assert float((path != path_t).float().mean()) <= 0.01


@pytest.mark.parametrize("copies", [3, 5])
def test_layer_trains_through_the_wide_kernels(copies, monkeypatch):
    """One training step with fused_training=True against the torch-op path; tolerance of test_emitter_grad_gpu's
    layer test."""
    b, L = 3, 200
    fwd_calls = count_calls(monkeypatch, "gene_emissions_wide")
    bwd_calls = count_calls(monkeypatch, "gene_emissions_grad_wide")

    def step(fused):
        cell, x = gene_cell(copies, b, L, 3, fused_training=fused)
        layer = MsaHmmLayer(cell, use_prior=False)
        layer.build(x.shape)
        xs = x.clone().requires_grad_(True)
        _, mean = layer(xs, training=True)
        (-mean).backward()
        torch.cuda.synchronize()
        return {n: p.grad.detach().clone() for n, p in cell.named_parameters() if p.grad is not None}, xs.grad.detach()

    got, gx = step(True)
    assert len(fwd_calls) == 1 and len(bwd_calls) == 1         # the fused node ran, forward and backward
    want, wx = step(False)
    assert len(fwd_calls) == 1 and len(bwd_calls) == 1
    assert set(got) == set(want) and any("emission_kernel" in n for n in got) and len(got) >= 2
    for n in want:
        scale = float(want[n].abs().max())
        err = float((got[n] - want[n]).abs().max())
        print("copies %d %s: scale %.4g err %.3g" % (copies, n, scale, err))
        assert err <= 5e-4 * scale + 1e-7, (n, err, scale)
    scale = float(wx[..., :S].abs().max())
    err = float((gx[..., :S] - wx[..., :S]).abs().max())
    print("copies %d x.grad (classes): scale %.4g err %.3g" % (copies, scale, err))
    assert err <= 5e-4 * scale + 1e-7, (err, scale)
    assert float(gx[..., S:].abs().max()) == 0.0
