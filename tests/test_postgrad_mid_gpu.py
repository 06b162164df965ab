"""hmm_posterior_grad for 17..64 states, the whole-sequence sweeps (csrc/hmm_postgrad.inc: k_pg_fb<QB>, k_pg_adj<QB>,
k_pg_merge, k_pg_grad_sum, k_pg_sum_rows with QB = 32, 48, 64), against the fp64 oracle.  Needs an MI355X.

Inputs, norms and limits: tests/postgrad_mid_cases.py (four norms: per tensor at the project's 3e-4, and dE per state
column, dE per sequence, dA per row over present edges at max(3e-4, 4 e32), e32 = the error of fp32 autograd through
the same recursion on the CPU).  tests/test_postgrad_mid_cpu.py shows from the oracle alone that the inputs can carry
this.  Every call runs with HMM_OPT_PGCHUNK = 0: the per-chunk path (29 states) has tests/test_postgrad_chunked_gpu.py.
Each comparison prints its figures (pytest -s) before it asserts.

Worst error / limit measured on an MI355X over all cases of this file, per norm, with the largest e32 of that norm:
    tensor   0.009  (2.7e-6 of 3e-4,    gene-q29-b3-L203-dead-label-log);    e32 <= 5.3e-6
    dE/col   0.48   (1.45e-4 of 3e-4,   gene-q29-b3-L203-dead-label-prob);   e32 <= 1.3e-4 (gene-q57-b3-L203-rare-label-log)
    dE/seq   0.013  (3.9e-6 of 3e-4,    gene+sparse-q43-b64-L24-holes-dense-prob);  e32 <= 1.6e-5
    dA/row   0.57   (1.76e-4 of 3.09e-4, gene-q43-b3-L203-holes-dense-prob); e32 <= 2.1e-4 (gene+sparse-q57-b2-L17-holes-dense-prob)
"""
import numpy as np
import pytest
import torch

from hmm_layer_amd import engine
from oracle import ref_cell, torch64

import postgrad_mid_cases as pc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CODONS = dict(start_codons=[("ATG", 1.)], stop_codons=[("TAG", .34), ("TAA", .33), ("TGA", .33)],
              intron_begin_pattern=[("NGT", .99), ("NGC", .005), ("NAT", .005)],
              intron_end_pattern=[("AGN", .99), ("ACN", .01)])


def dev(x):
    return torch.as_tensor(np.array(x, dtype=np.float32, order="C"), device=DEV)    # (a copy: the cases are read-only)


def run(A, pi, E, G, log):
    """numpy (k,q,q), (k,q), (k,b,L,q), (k,b,L,q) -> numpy dA, dpi, dE of the whole-sequence sweeps."""
    with engine.option(engine.OPT_PGCHUNK, 0):
        out = engine.posterior_grad(dev(A), dev(pi), dev(E), dev(G), mode=engine.POST_LOG if log else engine.POST_PROB)
        assert engine.posterior_grad_serial_count(E.shape) == E.shape[0] * E.shape[1]
    return [t.cpu().numpy() for t in out]


def check(spec, got=None):
    """The case on the engine against the oracle under the four norms -> (inputs, dA, dpi, dE, reference)."""
    c = pc.build(spec)
    ref = pc.reference(spec)
    got = got or run(c["A"], c["pi"], c["E"], c["G"], spec.log)
    failed = []
    for m, r in enumerate(ref):
        mine = [x[m] for x in got]
        assert all(np.isfinite(x).all() for x in mine), (pc.spec_id(spec), m)
        err, _ = pc.errors(mine, r["want"], c["A"][m])
        for norm, lim in pc.limits(r).items():
            print("PGMID %s m=%d %s err %.3e limit %.3e e32 %.3e" % (pc.spec_id(spec), m, norm, err[norm], lim, r["e32"][norm]))
            if not err[norm] <= lim:
                failed.append((m, norm, err[norm], lim))
        assert np.all(mine[2][c["E"][m] <= pc.EPS] == 0.0), (pc.spec_id(spec), m)     # clamped emissions: exactly 0
    assert not failed, (pc.spec_id(spec), failed)
    return c, got, ref


@pytest.mark.parametrize("spec", pc.state_sweep(), ids=pc.spec_id)
def test_state_sweep(spec):
    """q at both ends of and inside every QB block, the 29-, 43- and 57-state gene models; L = 203 = 25 prefetch blocks
    of 8 and a tail of 3; holes / rare / dead emissions."""
    c, got, _ = check(spec)
    if spec.emis in ("holes", "dead"):
        assert (c["E"] <= pc.EPS).any()


@pytest.mark.parametrize("spec", pc.length_sweep(), ids=pc.spec_id)
def test_length_sweep_two_models(spec):
    """L around one and two prefetch blocks, two different models in one call (m = row / b)."""
    c, got, _ = check(spec)
    if spec.L == 1:
        assert np.all(got[0] == 0.0)


@pytest.mark.parametrize("spec", pc.clamp_cases(), ids=pc.spec_id)
def test_clamped_recursions(spec):
    """The sign-bit flags of AH (forward clamp) and RB (backward clamp) at q = 40 (QB 48) and q = 60 (QB 64)."""
    c, got, ref = check(spec)
    if spec.models[0] == "fclamp":                           # the 1e-20 edge keeps what the backward recursion sends it
        D, rA = spec.q - 1, ref[0]["want"][0]
        assert c["A"][0, 0, D] > 0
        assert abs(got[0][0, 0, D] - rA[0, D]) <= 3e-4 * np.abs(rA).max()


@pytest.mark.parametrize("spec", pc.batch_sweep(), ids=pc.spec_id)
def test_batch_sweep_and_each_sequence_alone(spec):
    """b on both sides of the 64-lane stride of k_pg_grad_sum / k_pg_sum_rows, two models; a sequence's dE is that of
    the sequence run alone, bit for bit (one wave pair per sequence, nothing shared)."""
    c, got, _ = check(spec)
    for s in range(spec.b):
        alone = run(c["A"], c["pi"], c["E"][:, s:s + 1], c["G"][:, s:s + 1], spec.log)
        assert np.array_equal(alone[2][:, 0], got[2][:, s]), s


@pytest.mark.parametrize("log", pc.MODES)
def test_workspace_reuse(log):
    """The engine keeps its workspace between calls: a small case, a larger one (the workspace grows), the small one
    again."""
    X = [s for s in pc.length_sweep() if (s.q, s.L, s.log) == (43, 9, log)][0]
    Y = [s for s in pc.batch_sweep() if (s.b, s.log) == (130, log)][0]
    x, y = pc.build(X), pc.build(Y)
    engine.release_workspaces()
    first = run(x["A"], x["pi"], x["E"], x["G"], log)
    check(Y)
    again = run(x["A"], x["pi"], x["E"], x["G"], log)
    for a, b in zip(first, again):
        assert np.array_equal(a, b)
    check(X, again)


@pytest.mark.parametrize("q,kind", [(43, "gene"), (57, "sparse")])
def test_no_loglik_variant_through_the_autograd_node(q, kind):
    """out = log gamma + loglik (POST_LOG_NO_LL): posterior gradient + weighted log-likelihood gradient; tolerance
    and masking of tests/test_postgrad_gpu.py::test_no_loglik_variant_through_the_autograd_node."""
    from hmm_layer_amd import autograd
    rng = np.random.default_rng(23 + q)
    A, pi = pc.gene_model(pc.copies_of(q)) if kind == "gene" else pc.rand_model(rng, q, sparse=True)
    E = (rng.random((1, 3, 80, q)) * 0.9 + 0.05).astype(np.float32)
    G = rng.standard_normal(E.shape).astype(np.float32)
    At, pit, Et = dev(A)[None].requires_grad_(True), dev(pi)[None].requires_grad_(True), dev(E).requires_grad_(True)
    out = autograd.posterior(At, pit, Et, mode=engine.POST_LOG_NO_LL)
    (out * dev(G)).sum().backward()
    rA, rpi, rE, rout = torch64.posterior_grad(np.array(A), np.array(pi), E[0], G[0], log=True, add_loglik=True)
    g64, _ = torch64.posterior(torch.tensor(np.array(A), dtype=torch.float64), torch.tensor(np.array(pi), dtype=torch.float64),
                               torch.tensor(E[0], dtype=torch.float64))
    m = g64.numpy() > 1e-4              # log space only where eps-clamp paths cannot dominate the value
    assert np.abs(out.detach().cpu().numpy()[0] - rout)[m].max() <= 2e-3
    for got, want in ((At.grad[0], rA), (pit.grad[0], rpi), (Et.grad[0], rE)):
        assert np.abs(got.cpu().numpy() - want).max() <= 3e-4 * np.abs(want).max() + 1e-6


@pytest.mark.parametrize("copies", [3, 4])
def test_layer_trained_through_state_posteriors(copies):
    """A cross-entropy on layer.state_posterior_log_probs(x, training=True) for the 43- and 57-state models,
    back-propagated by the engine; parameter gradients against autograd through the restated reference loops on the
    CPU (structure and tolerance of test_five_copy_layer_trained_through_state_posteriors)."""
    from hmm_layer_amd.MsaHmmCell import HmmCell
    from hmm_layer_amd.MsaHMMLayer import MsaHmmLayer
    from hmm_layer_amd.gene_pred_hmm_emitter import GenePredHMMEmitter
    from hmm_layer_amd.gene_pred_hmm_transitioner import GenePredMultiHMMTransitioner
    b, L, q = 2, 160, 1 + 14 * copies
    g = torch.Generator().manual_seed(13 + copies)
    cls = torch.softmax(2 * torch.randn((1, b, L, 15), generator=g), -1)
    nuc = torch.nn.functional.one_hot(torch.randint(0, 4, (1, b, L), generator=g), 5).float()
    x = torch.cat([cls, nuc], -1).to(DEV)
    target = torch.softmax(torch.randn((1, b, L, q), generator=g), -1)
    em = GenePredHMMEmitter(**CODONS, num_copies=copies)
    em.build((1, b, L, 15))
    tr = GenePredMultiHMMTransitioner(k=copies, initial_exon_len=200, initial_intron_len=4500, initial_ir_len=10000)
    cell = HmmCell([q], 15, em, tr).to(DEV)
    layer = MsaHmmLayer(cell, use_prior=False)
    layer.build(x.shape)
    logp = layer.state_posterior_log_probs(x, training=True)
    assert logp.requires_grad
    loss = -(target.to(DEV) * logp).sum() / (b * L)
    loss.backward()
    plist = [(n, p) for n, p in cell.named_parameters() if p.grad is not None]
    got = {n: p.grad.detach().clone() for n, p in plist}
    # reference mechanism: autograd through the restated loops on the CPU, then back through the cell's own ops
    cell.recurrent_init()
    E = cell.emission_probs(x, end_hints=None, training=True).to(torch.float32)
    A, pi = cell.A, cell.init_dist.reshape(1, q)
    Ac, pic, Ec = [t.detach().cpu().requires_grad_(True) for t in (A, pi, E)]
    lp = ref_cell.posterior_log_probs(ref_cell.HmmParams(Ac, pic), Ec)
    lp = lp[0] if isinstance(lp, tuple) else lp
    ref_loss = -(target * lp).sum() / (b * L)
    assert abs(float(loss.detach()) - float(ref_loss.detach())) <= 1e-4 * abs(float(ref_loss.detach())) + 1e-4
    dA, dpi, dE = torch.autograd.grad(ref_loss, [Ac, pic, Ec], allow_unused=True)
    outs = [(A, dA), (pi, dpi), (E, dE)]
    outs = [(t, d) for t, d in outs if d is not None]
    want = torch.autograd.grad([t for t, _ in outs], [p for _, p in plist], [d.to(DEV) for _, d in outs],
                               allow_unused=True)
    checked = 0
    for (n, _), wt in zip(plist, want):
        if wt is None:
            continue
        scale = float(wt.abs().max())
        assert float((got[n] - wt).abs().max()) <= 2e-3 * scale + 1e-7, (n, float((got[n] - wt).abs().max()), scale)
        checked += 1
    assert checked >= 2
