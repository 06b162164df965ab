"""hmm_posterior_grad_large (engine.posterior_grad_large, q up to 4096): gradient of a loss on the state posteriors,
under both evaluations (HMM_OPT_GLARGE = 1 per-sequence walk where q <= 128, 2 per-position GEMMs) and the default (0).

Oracle: torch autograd in float64 through oracle/torch64.py, as in tests/test_postgrad_gpu.py, with its tolerance:
|g - g64| <= 3e-4 * max|g64| per tensor (fp32 serial recursions over L steps; the log mode divides by small
posteriors)."""
import numpy as np
import pytest
import torch

from hmm_layer_amd import engine
from oracle import ref_cell, torch64

import largeq_grad_cases as lg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WALK_MAX = 128
MODES = (engine.POST_PROB, engine.POST_LOG)
CODONS = dict(start_codons=[("ATG", 1.)], stop_codons=[("TAG", .34), ("TAA", .33), ("TGA", .33)],
              intron_begin_pattern=[("NGT", .99), ("NGC", .005), ("NAT", .005)],
              intron_end_pattern=[("AGN", .99), ("ACN", .01)])


def dev(x):
    return torch.as_tensor(np.asarray(x), dtype=torch.float32, device=DEV)


def routes(q):
    return (1, 2) if q <= WALK_MAX else (2,)


def run(A, pi, E, G, mode, route=0, fn=None):
    """numpy (k,q,q), (k,q), (k,b,L,q), (k,b,L,q) -> numpy dA, dpi, dE under OPT_GLARGE = route."""
    fn = fn or engine.posterior_grad_large
    with engine.option(engine.OPT_GLARGE, route):
        out = fn(dev(A), dev(pi), dev(E), dev(G), mode=mode)
        torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def check_model(got, A, pi, E, G, mode, tag):
    """got = (dA, dpi, dE) of ONE model, E and G (b,L,q)."""
    rA, rpi, rE, _ = torch64.posterior_grad(A, pi, E, G, log=(mode == engine.POST_LOG))
    dA, dpi, dE = got
    for x, want, name in ((dA, rA, "dA"), (dpi, rpi, "dpi"), (dE, rE, "dE")):
        assert np.isfinite(x).all(), (tag, name)
        assert np.abs(x - want).max() <= 3e-4 * np.abs(want).max() + 1e-6, \
            (tag, name, np.abs(x - want).max(), np.abs(want).max())
    return rA, rpi, rE


def check_all(A, pi, E, G, tag=""):
    """Every route and both modes, each model against the oracle."""
    res = {}
    for mode in MODES:
        for r in routes(E.shape[-1]):
            got = run(A, pi, E, G, mode, r)
            res[mode, r] = got
            for m in range(E.shape[0]):
                check_model([x[m] for x in got], A[m], pi[m], E[m], G[m], mode, "%s mode=%d route=%d m=%d" % (tag, mode, r, m))
    return res


def rand_model(rng, q, sparse=False, dead=0, tiny_pi=0):
    """Row-stochastic A; `dead` states nothing enters; `tiny_pi` entries of pi below eps."""
    A = rng.random((q, q)) ** 2 + 1e-2
    if sparse:
        A *= rng.random((q, q)) < 0.1
        A += np.eye(q) * 0.3
        A[np.arange(q), (np.arange(q) + 1) % q] += 0.2
    if dead:
        A[:, q - dead:] = 0.0
        A[q - dead:, q - dead:] = np.eye(dead) * 0.5
        A[q - dead:, 0] += 0.5
    A /= A.sum(-1, keepdims=True)
    pi = rng.random(q) + 0.1
    if tiny_pi:
        pi[rng.choice(q, tiny_pi, replace=False)] = 1e-20
    pi /= pi.sum()
    return A.astype(np.float32), pi.astype(np.float32)


def rand_E(rng, k, b, L, q, holes=True):
    E = (rng.random((k, b, L, q)) * 0.9 + 0.05).astype(np.float32)
    if holes:
        E[..., ::5, q // 3] = 0.0                        # emissions below eps: no gradient there
    return E


def rand_G(rng, shape):
    return rng.standard_normal(shape).astype(np.float32)


def five_copy():
    from hmm_layer_amd.gene_pred_hmm_transitioner import GenePredMultiHMMTransitioner
    tr = GenePredMultiHMMTransitioner(k=5, initial_exon_len=200, initial_intron_len=4500, initial_ir_len=10000)
    with torch.no_grad():
        A = tr.make_A()[0].numpy().astype(np.float32)
        pi = tr.make_initial_distribution().reshape(-1).numpy().astype(np.float32)
    return A, pi


@pytest.mark.parametrize("q,kind", [(65, "dense"), (100, "sparse"), (127, "dense"), (128, "sparse"), (129, "dense"),
                                    (257, "sparse")])
def test_models_against_the_oracle(q, kind):
    rng = np.random.default_rng(q)
    A, pi = rand_model(rng, q, sparse=kind == "sparse", dead=3, tiny_pi=2)
    E = rand_E(rng, 1, 3, 40, q)
    check_all(A[None], pi[None], E, rand_G(rng, E.shape), "q=%d %s" % (q, kind))


def test_five_copy_gene_model():
    rng = np.random.default_rng(71)
    A, pi = five_copy()
    assert A.shape == (71, 71)
    E = rand_E(rng, 1, 3, 300, 71)
    check_all(A[None], pi[None], E, rand_G(rng, E.shape), "five-copy")


@pytest.mark.parametrize("b,q,L,cols", [(1024, 1027, 3, 80), (3328, 344, 2, 96), (192, 1027, 3, 64)])
def test_config5_shape_and_every_gemm_tile(b, q, L, cols):
    """BASELINE config 5's model size and batch (q = 1027, b = 1024) and shapes selecting the other GEMM tile widths:
    the full dA and dpi, dE of sampled sequences (sequences are independent rows of every GEMM)."""
    assert engine.largeq_tile_cols(b, q) == cols
    rng = np.random.default_rng(q + b)
    A, pi = rand_model(rng, q, sparse=True, dead=4, tiny_pi=5)
    E = rand_E(rng, 1, b, L, q)
    G = rand_G(rng, E.shape)
    rows = [0, 1, b // 2, b - 1]
    for mode in MODES:
        dA, dpi, dE = run(A[None], pi[None], E, G, mode)
        rA, rpi, _, _ = torch64.posterior_grad(A, pi, E[0], G[0], log=(mode == engine.POST_LOG))
        rE = torch64.posterior_grad(A, pi, E[0, rows], G[0, rows], log=(mode == engine.POST_LOG))[2]
        for x, want, name in ((dA[0], rA, "dA"), (dpi[0], rpi, "dpi"), (dE[0, rows], rE, "dE")):
            assert np.isfinite(x).all(), name
            assert np.abs(x - want).max() <= 3e-4 * np.abs(want).max() + 1e-6, (mode, name, np.abs(x - want).max())


def test_two_models_short_sequences_and_labels():
    """k = 2 with separate matrices, L = 1..7 (L = 1: dA exactly 0), label-like upstream gradients in log mode; then
    the whole first row of each model's sequence 3 blank, under the finer norms of tests/largeq_grad_cases.py as
    well."""
    rng = np.random.default_rng(5)
    q = 90
    m1, m2 = rand_model(rng, q, dead=2), rand_model(rng, q, sparse=True, tiny_pi=3)
    A, pi = np.stack([m1[0], m2[0]]), np.stack([m1[1], m2[1]])
    for L in range(1, 8):
        E = rand_E(rng, 2, 5, L, q)
        res = check_all(A, pi, E, rand_G(rng, E.shape), "L=%d" % L)
        if L == 1:
            for r in res.values():
                assert np.all(r[0] == 0.0)
        G = -(rng.random(E.shape) < 0.05).astype(np.float32)                   # cross-entropy against labels
        for r in routes(q):
            got = run(A, pi, E, G, engine.POST_LOG, r)
            for m in range(2):
                check_model([x[m] for x in got], A[m], pi[m], E[m], G[m], engine.POST_LOG, "labels L=%d r=%d" % (L, r))
        E0, G0 = E.copy(), rand_G(np.random.default_rng(50 + L), E.shape)      # (a generator of its own: the draws above stay)
        E0[:, 3, 0, :] = 0.0
        for (mode, r), got in check_all(A, pi, E0, G0, "blank0 L=%d" % L).items():
            for m in range(2):
                lg.post_fine_check([x[m] for x in got], A[m], pi[m], E0[m], G0[m], mode == engine.POST_LOG,
                                   "blank0 L=%d mode=%d route=%d m=%d" % (L, mode, r, m))


@pytest.mark.parametrize("q", [70, 150])
def test_clamped_predicted_state(q):
    """A state on the eps floor at every position, entered by a PRESENT edge of weight 1e-20 and emitting with
    probability 1: the forward cell clamps its predicted mass at every step, so the forward adjoint passes nothing
    through it.  The edge's dA entry keeps what the backward recursion sends it (Rb_t[0] reads bh_{t+1} of that
    state), and must match the oracle."""
    rng = np.random.default_rng(q)
    D = q - 1
    A = rng.random((q, q)) ** 2 + 1e-2
    A[:, D] = 0.0
    A[0, D] = 1e-20
    A[D, :] = 0.0
    A[D, 0] = 1.0
    A /= A.sum(-1, keepdims=True)
    pi = rng.random(q) + 0.1
    pi[D] = 0.0
    pi /= pi.sum()
    A, pi = A.astype(np.float32), pi.astype(np.float32)
    E = (rng.random((1, 3, 60, q)) * 0.9 + 0.05).astype(np.float32)
    E[..., D] = 1.0
    G = rand_G(rng, E.shape)
    for mode in MODES:
        for r in routes(q):
            got = run(A[None], pi[None], E, G, mode, r)
            rA = check_model([x[0] for x in got], A, pi, E[0], G[0], mode, "floor q=%d mode=%d route=%d" % (q, mode, r))[0]
            assert abs(got[0][0, 0, D] - rA[0, D]) <= 3e-4 * np.abs(rA).max()


@pytest.mark.parametrize("q", [71, 200])
def test_rare_emissions_on_the_most_probable_path(q):
    """A fifth of the emissions are 1e-10 (far above eps: nothing is clamped); labels = the most probable state."""
    rng = np.random.default_rng(31 + q)
    A, pi = five_copy() if q == 71 else rand_model(rng, q, sparse=True)
    E = (rng.random((1, 2, 400, q)) * 0.9 + 0.05).astype(np.float32)
    rare = rng.random(E.shape) < 0.2
    rare[..., :6] = False
    E[rare] = 1e-10
    gam, _ = engine.posterior(dev(A)[None], dev(pi)[None], dev(E))
    G = -(gam == gam.amax(-1, keepdim=True)).float().cpu().numpy()
    for mode in MODES:
        for r in routes(q):
            got = run(A[None], pi[None], E, G, mode, r)
            check_model([x[0] for x in got], A, pi, E[0], G[0], mode, "rare q=%d mode=%d route=%d" % (q, mode, r))


@pytest.mark.parametrize("q", [1, 15, 29, 33, 43, 48, 57, 64])
def test_equals_hmm_posterior_grad_up_to_64_states(q):
    rng = np.random.default_rng(100 + q)
    A, pi = rand_model(rng, q, sparse=q % 2 == 1)
    E = rand_E(rng, 1, 4, 120, q, holes=q > 2)
    G = rand_G(rng, E.shape)
    for mode in MODES:
        with engine.option(engine.OPT_PGCHUNK, 0):
            old = run(A[None], pi[None], E, G, mode, fn=engine.posterior_grad)
        for r in (0, 1, 2):
            got = run(A[None], pi[None], E, G, mode, r)
            for x, y, name in zip(got, old, ("dA", "dpi", "dE")):
                # (q = 1: gamma is 1 and every gradient is zero up to rounding, hence the absolute floor)
                assert np.abs(x - y).max() <= 1e-4 * np.abs(y).max() + 2e-6, (q, mode, r, name, np.abs(x - y).max())


def test_default_route_switches_at_128_states():
    rng = np.random.default_rng(128)
    for q, route in ((128, 1), (129, 2)):
        A, pi = rand_model(rng, q, dead=2)
        E = rand_E(rng, 1, 6, 30, q)
        G = rand_G(rng, E.shape)
        d0, dr = run(A[None], pi[None], E, G, engine.POST_LOG, 0), run(A[None], pi[None], E, G, engine.POST_LOG, route)
        for x, y in zip(d0, dr):
            assert np.array_equal(x, y), q


@pytest.mark.parametrize("q,route", [(71, 1), (71, 2), (300, 2)])
def test_deterministic(q, route):
    rng = np.random.default_rng(q + route)
    A, pi = rand_model(rng, q, sparse=True, dead=2)
    E = rand_E(rng, 1, 200, 30, q)
    G = rand_G(rng, E.shape)
    for mode in MODES:
        a = run(A[None], pi[None], E, G, mode, route)
        b = run(A[None], pi[None], E, G, mode, route)
        for x, y in zip(a, b):
            assert np.array_equal(x, y)


def test_offsets_beyond_2_to_31():
    """k*b*L*q > 2^31 elements (E, grad_out, dE and the stored values beyond 8 GB): sampled sequences, the last
    included, under both evaluations.  A sequence's dE depends on that sequence alone, so the yardstick is the same
    call on the sampled sequences by themselves (offsets far below 2^31; the other tests hold that call to the fp64
    oracle, whose per-position indexing makes its own cost grow as L^2 at this length)."""
    k, b, L, q = 1, 1024, 30000, 71
    assert k * b * L * q > 2 ** 31
    A, pi = five_copy()
    gen = torch.Generator(device=DEV).manual_seed(9)
    E = torch.rand((k, b, L, q), generator=gen, device=DEV) * 0.9 + 0.05
    G = torch.randn((k, b, L, q), generator=gen, device=DEV)
    rows = [0, 517, b - 1]
    Es, Gs = E[:, rows].contiguous(), G[:, rows].contiguous()
    for r in (1, 2):
        with engine.option(engine.OPT_GLARGE, r):
            dA, dpi, dE = engine.posterior_grad_large(dev(A[None]), dev(pi[None]), E, G, mode=engine.POST_LOG)
            want = engine.posterior_grad_large(dev(A[None]), dev(pi[None]), Es, Gs, mode=engine.POST_LOG)[2]
            torch.cuda.synchronize()
        assert bool(torch.isfinite(dA).all()) and bool(torch.isfinite(dpi).all())
        assert bool(torch.isfinite(dE[0, -1]).all()) and bool(torch.isfinite(dE[0, :, -1]).all())
        got, want = dE[0, rows].cpu().numpy(), want[0].cpu().numpy()
        if r == 1:                                       # the walk: one workgroup per sequence, whatever the batch
            assert np.array_equal(got, want)
        assert np.abs(got - want).max() <= 3e-4 * np.abs(want).max(), (r, np.abs(got - want).max())
        del dA, dpi, dE
    del E, G
    torch.cuda.empty_cache()


def test_routing_and_limits():
    A, pi = rand_model(np.random.default_rng(0), 129)
    E = rand_E(np.random.default_rng(1), 1, 2, 5, 129)
    with engine.option(engine.OPT_GLARGE, 1):
        with pytest.raises(engine.EngineError):          # the forced walk above 128 states: HMM_ERR_BAD_ARGUMENT
            engine.posterior_grad_large(dev(A[None]), dev(pi[None]), dev(E), dev(E))
    with pytest.raises(ValueError):                      # the old entry point keeps its limit
        engine.posterior_grad(torch.eye(70, device=DEV)[None], torch.full((1, 70), 1 / 70, device=DEV),
                              torch.rand(1, 2, 8, 70, device=DEV), torch.rand(1, 2, 8, 70, device=DEV))
    with pytest.raises(ValueError):
        z = torch.zeros(1, 1, 1, 4097, device=DEV)
        engine.posterior_grad_large(torch.zeros(1, 4097, 4097, device=DEV), torch.zeros(1, 4097, device=DEV), z, z)
    with pytest.raises(ValueError):
        engine.posterior_grad_large(dev(A[None]), dev(pi[None]), dev(E), dev(E), mode=engine.POST_LOG_NO_LL)


@pytest.mark.parametrize("mode", [engine.POST_PROB, engine.POST_LOG, engine.POST_LOG_NO_LL])
def test_autograd_node_above_64_states(mode):
    from hmm_layer_amd import autograd
    rng = np.random.default_rng(23 + mode)
    for q in (80, 160):
        A, pi = rand_model(rng, q, sparse=True)
        E = (rng.random((1, 3, 50, q)) * 0.9 + 0.05).astype(np.float32)
        G = rand_G(rng, E.shape)
        At, pit, Et = dev(A)[None].requires_grad_(True), dev(pi)[None].requires_grad_(True), dev(E).requires_grad_(True)
        out = autograd.posterior(At, pit, Et, mode=mode)
        (out * dev(G)).sum().backward()
        rA, rpi, rE, _ = torch64.posterior_grad(A, pi, E[0], G[0], log=mode != engine.POST_PROB,
                                                add_loglik=mode == engine.POST_LOG_NO_LL)
        for got, want in ((At.grad[0], rA), (pit.grad[0], rpi), (Et.grad[0], rE)):
            assert np.abs(got.cpu().numpy() - want).max() <= 3e-4 * np.abs(want).max() + 1e-6, (q, mode)


def test_five_copy_layer_trained_through_state_posteriors():
    """A cross-entropy on layer.state_posterior_log_probs(x, training=True) for the 71-state model, back-propagated by
    the engine; parameter gradients against autograd through the restated reference loops on the CPU."""
    from hmm_layer_amd.MsaHmmCell import HmmCell
    from hmm_layer_amd.MsaHMMLayer import MsaHmmLayer
    from hmm_layer_amd.gene_pred_hmm_emitter import GenePredHMMEmitter
    from hmm_layer_amd.gene_pred_hmm_transitioner import GenePredMultiHMMTransitioner
    b, L, q = 2, 160, 71
    g = torch.Generator().manual_seed(13)
    cls = torch.softmax(2 * torch.randn((1, b, L, 15), generator=g), -1)
    nuc = torch.nn.functional.one_hot(torch.randint(0, 4, (1, b, L), generator=g), 5).float()
    x = torch.cat([cls, nuc], -1).to(DEV)
    target = torch.softmax(torch.randn((1, b, L, q), generator=g), -1)
    em = GenePredHMMEmitter(**CODONS, num_copies=5)
    em.build((1, b, L, 15))
    tr = GenePredMultiHMMTransitioner(k=5, initial_exon_len=200, initial_intron_len=4500, initial_ir_len=10000)
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
