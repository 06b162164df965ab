"""hmm_gene_emissions_grad on a HIP device: the backward of the fused gene emitter against torch autograd through
GenePredHMMEmitter.forward on an fp64 CPU copy of the module, the node's options, and the layer trained through
it against the torch-op path.  Needs an MI355X.

Tolerance of the kernel tests: per case the fp32 torch path is run on the CPU too; e32 is its error against fp64.
The kernel must satisfy max|got - ref| <= max(4 e32, 2e-6 max|ref|) for dx (class columns) and for
d emission_kernel (dB chained through the softmax) — the factor 4 covers another summation order over the
positions, nothing else."""
import copy
import functools

import pytest
import torch

from hmm_layer_amd import engine
from hmm_layer_amd.MsaHmmCell import HmmCell
from hmm_layer_amd.MsaHMMLayer import MsaHmmLayer, _loglik_impl
from hmm_layer_amd.gene_pred_hmm_emitter import GenePredHMMEmitter
from hmm_layer_amd.gene_pred_hmm_transitioner import GenePredMultiHMMTransitioner

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CODONS = dict(start_codons=[("ATG", 1.)], stop_codons=[("TAG", .34), ("TAA", .33), ("TGA", .33)],
              intron_begin_pattern=[("NGT", .99), ("NGC", .005), ("NAT", .005)],
              intron_end_pattern=[("AGN", .99), ("ACN", .01)])
SHAPES = [(3, 5), (7, 16), (4, 37), (2, 1100), (5, 4099)]
# name -> (emitter arguments, classes, training)
MODELS = {
    "default": (dict(), 15, True),
    "default_inference": (dict(), 15, False),
    "s7": (dict(), 7, True),
    "s20": (dict(), 20, True),
    "copies2_unshared": (dict(num_copies=2, share_intron_parameters=False), 15, True),
    "copies2_shared": (dict(num_copies=2), 15, True),
    "n_mass_compat": (dict(n_mass_compat=True), 15, True),
}


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
    kw, s, training = MODELS[model]
    g = torch.Generator().manual_seed(1000 * b + L + 7 * s + int(soft))
    x = make_inputs(b, L, s, soft, g)
    em = GenePredHMMEmitter(**CODONS, **kw)
    em.build((1, b, L, s))
    with torch.no_grad():
        em.emission_kernel.copy_(torch.randn(em.emission_kernel.shape, generator=g))
    G = torch.randn((1, b, L, em.num_states), generator=g)
    ref_dx, ref_dk = torch_grads(copy.deepcopy(em).double(), x.double(), G.double(), training)
    c32_dx, c32_dk = torch_grads(copy.deepcopy(em), x, G, training)
    dev = copy.deepcopy(em).to(DEV)
    xd = x.to(DEV).requires_grad_(True)
    assert dev.can_fuse(xd)
    E = dev.forward_fused_trainable(xd, training=training)
    (E * G.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    return dict(s=s, ref_dx=ref_dx, ref_dk=ref_dk, c32_dx=c32_dx.double(), c32_dk=c32_dk.double(),
                got_dx=xd.grad.detach().cpu().double(), got_dk=dev.emission_kernel.grad.detach().cpu().double(),
                em=em, x=x, G=G, training=training)


def check_case(c, tag):
    s = c["s"]
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
def test_kernel_against_fp64_autograd(model, b, L):
    check_case(case(model, b, L), "%s (%d, %d)" % (model, b, L))


@pytest.mark.parametrize("b,L", [(4, 37), (2, 1100)])
@pytest.mark.parametrize("model", ["default", "n_mass_compat", "copies2_shared"])
def test_kernel_soft_nucleotides(model, b, L):
    """The generic path: soft rows, N flags that are not exactly 1, N next to a base."""
    check_case(case(model, b, L, True), "%s soft (%d, %d)" % (model, b, L))


def engine_args(c):
    em = copy.deepcopy(c["em"]).to(DEV)
    row, cod = em.state_tables(torch.device(DEV))
    with torch.no_grad():
        B = em.make_B()[0].contiguous()
    kw = dict(add=1e-7 if c["training"] else 0.0, n_mass=2 if em.n_mass_compat else 1)
    return (c["x"][0].to(DEV).contiguous(), B, row, em.codon_probs.to(DEV, torch.float32).contiguous(), cod), kw


@pytest.mark.parametrize("model,b,L", [("default", 5, 4099), ("copies2_shared", 2, 1100), ("s20", 4, 37)])
def test_outputs_alone_and_repeated_are_bit_identical(model, b, L):
    c = case(model, b, L)
    args, kw = engine_args(c)
    G = c["G"][0].to(DEV).contiguous()
    dx, dB = engine.gene_emissions_grad(*args, G, **kw)
    dx2, dB2 = engine.gene_emissions_grad(*args, G, **kw)
    assert torch.equal(dx, dx2) and torch.equal(dB, dB2)
    only_dx, none = engine.gene_emissions_grad(*args, G, want_dB=False, **kw)
    assert none is None and torch.equal(only_dx, dx)
    none, only_dB = engine.gene_emissions_grad(*args, G, want_dx=False, **kw)
    assert none is None and torch.equal(only_dB, dB)
    assert engine.gene_emissions_grad(*args, G, want_dx=False, want_dB=False, **kw) == (None, None)
    # the node's result is the direct call's
    assert torch.equal(dx.cpu().double(), c["got_dx"][0])


@pytest.mark.parametrize("model,b,L,at", [("default", 2, 1100, (0, 1023)), ("default", 2, 1100, (1, 0)),
                                          ("copies2_unshared", 4, 37, (2, 36)), ("s7", 7, 16, (3, 15))])
def test_gradient_at_one_position_stays_there(model, b, L, at):
    c = case(model, b, L)
    args, kw = engine_args(c)
    G = torch.zeros_like(c["G"][0])
    G[at] = c["G"][0][at]
    dx, dB = engine.gene_emissions_grad(*args, G.to(DEV), **kw)
    nz = dx.abs().sum(-1).cpu()
    assert float(nz[at]) > 0
    nz[at] = 0
    assert float(nz.max()) == 0.0
    assert bool(torch.isfinite(dB).all()) and float(dB.abs().max()) > 0


def test_state_row_out_of_range_is_clamped():
    """The test of the same name in test_emitter_wide_gpu on the 64-state entry points: entries of state_row below 0
    or from rows on read row 0 / rows - 1 of B, in the forward and in both outputs of the backward."""
    q, rows, s, nc, b, L = 29, 20, 15, 9, 3, 150
    g = torch.Generator().manual_seed(5)
    x = make_inputs(b, L, s, False, g)[0]
    B = torch.softmax(torch.randn((rows, s), generator=g), -1)
    row = torch.randint(0, rows, (q,), generator=g, dtype=torch.int32)
    codon = torch.rand((2, nc, 64), generator=g) * (torch.rand((2, nc, 64), generator=g) < 0.5)
    cod = torch.randint(-1, nc, (q,), generator=g, dtype=torch.int32)
    bad_row = row.clone()
    bad_row[3], bad_row[17], bad_row[28] = -7, 20, 1 << 20
    row[3], row[17], row[28] = 0, 19, 19
    dE = torch.randn((b, L, q), generator=g).to(DEV)
    a = [t.to(DEV) for t in (x, B, row, codon, cod)]
    bad = [t.to(DEV) for t in (x, B, bad_row, codon, cod)]
    assert torch.equal(engine.gene_emissions(*a), engine.gene_emissions(*bad))
    for u, v in zip(engine.gene_emissions_grad(*a, dE), engine.gene_emissions_grad(*bad, dE)):
        assert torch.equal(u, v)


# ------------------------------------------------------------------------------------------------ layer level

def gene_cell(b, L, seed, fused, **kw):
    g = torch.Generator().manual_seed(seed)
    cls = torch.softmax(2 * torch.randn((1, b, L, 15), generator=g), -1)
    nuc = torch.nn.functional.one_hot(torch.randint(0, 5, (1, b, L), generator=g), 5).float()
    x = torch.cat([cls, nuc], -1)
    em = GenePredHMMEmitter(**CODONS, fused_training=fused, **kw)
    em.build((1, b, L, 15))
    with torch.no_grad():
        em.emission_kernel.copy_(torch.randn(em.emission_kernel.shape, generator=g))
    tr = GenePredMultiHMMTransitioner(initial_exon_len=200, initial_intron_len=4500, initial_ir_len=10000)
    return HmmCell([15], 15, em, tr).to(DEV), x.to(DEV)


def layer_step(fused, what, hints, b=3, L=400, seed=3):
    """One training step through the layer; -> (parameter gradients, x.grad, peak bytes allocated during the step)."""
    cell, x = gene_cell(b, L, seed, fused)
    layer = MsaHmmLayer(cell, use_prior=False)
    layer.build(x.shape)
    g = torch.Generator().manual_seed(77)
    W = torch.rand((1, b, L, 15), generator=g).to(DEV)
    end_hints = None
    if hints:
        end_hints = (0.25 + 0.75 * torch.rand((1, b, 2, 15), generator=g)).to(DEV)

    def step():
        xs = x.clone().requires_grad_(True)
        cell.zero_grad(set_to_none=True)
        if what == "loglik" and end_hints is None:
            _, mean = layer(xs, training=True)
            (-mean).backward()
        elif what == "loglik":                          # MsaHmmLayer.forward takes no end hints: the function under it
            (-_loglik_impl(xs, cell, end_hints=end_hints, training=True).mean()).backward()
        else:
            post = layer.state_posterior_log_probs(xs, end_hints=end_hints, training=True)
            (post * W).sum().backward()
        torch.cuda.synchronize()
        return xs

    step()                                              # workspaces of the recursions are cached from here on
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    xs = step()
    peak = torch.cuda.max_memory_allocated() - base
    grads = {n: p.grad.detach().clone() for n, p in cell.named_parameters() if p.grad is not None}
    return grads, xs.grad.detach().clone(), peak


@pytest.mark.parametrize("hints", [False, True])
@pytest.mark.parametrize("what", ["loglik", "posterior"])
def test_layer_trains_through_fused_emitter(what, hints):
    got, gx, peak_fused = layer_step(True, what, hints)
    want, wx, peak_torch = layer_step(False, what, hints)
    assert set(got) == set(want) and any("emission_kernel" in n for n in got) and len(got) >= 2
    for n in want:
        scale = float(want[n].abs().max())
        err = float((got[n] - want[n]).abs().max())
        print("%s hints=%s %s: scale %.4g err %.3g" % (what, hints, n, scale, err))
        assert err <= 5e-4 * scale + 1e-7, (n, err, scale)
    scale = float(wx[..., :15].abs().max())
    err = float((gx[..., :15] - wx[..., :15]).abs().max())
    print("%s hints=%s x.grad (classes): scale %.4g err %.3g; peak bytes fused %d torch %d"
          % (what, hints, scale, err, peak_fused, peak_torch))
    assert err <= 5e-4 * scale + 1e-7, (err, scale)
    assert float(gx[..., 15:].abs().max()) == 0.0
    assert peak_fused < peak_torch, (peak_fused, peak_torch)


def test_frozen_kernel_and_inputs_without_grad():
    cell, x = gene_cell(3, 400, 5, True, trainable_emissions=False)
    layer = MsaHmmLayer(cell, use_prior=False)
    layer.build(x.shape)
    xs = x.clone().requires_grad_(True)
    _, mean = layer(xs, training=True)
    (-mean).backward()
    assert cell.emitter[0].emission_kernel.grad is None
    assert xs.grad is not None and float(xs.grad[..., :15].abs().max()) > 0
    assert cell.transitioner.transition_kernel.grad is not None

    cell, x = gene_cell(3, 400, 5, True)
    layer = MsaHmmLayer(cell, use_prior=False)
    layer.build(x.shape)
    _, mean = layer(x, training=True)                  # inputs do not require grad
    (-mean).backward()
    assert x.grad is None
    gk = cell.emitter[0].emission_kernel.grad
    assert gk is not None and bool(torch.isfinite(gk).all()) and float(gk.abs().max()) > 0
