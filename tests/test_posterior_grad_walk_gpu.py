"""hmm_posterior_grad_walk (engine.posterior_grad_walk, 65..256 states, the per-sequence walk with the sparse step) on
the device: every case of tests/posterior_grad_walk_cases.py against the fp64 oracle under the project's four norms
(that module's docstring; nothing in a limit comes from engine output), exact zeros in dA wherever A == 0, and the
properties the header promises: a repeated call on a workspace of NaN bytes bit-identical, k = 2 bit-identical to two
k = 1 calls, the refusal of a model outside the sparse rule next to a served one, offsets beyond 2^31 elements, graph
capture, the autograd node (autograd.posterior(support_only=...)) and the five-copy layer."""
import ctypes

import numpy as np
import pytest
import torch

from hmm_layer_amd import autograd, engine

import loglik_grad_cases as lc
import posterior_grad_walk_cases as pc
import postgrad_mid_cases as pm
from test_loglik_grad_large_gpu import CODONS, five_copy

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(x):
    return torch.as_tensor(np.asarray(x), dtype=torch.float32, device=DEV)


def mode_of(log):
    return engine.POST_LOG if log else engine.POST_PROB


def run(A, pi, E, G, log, eps=pc.EPS, fn=None, **kw):
    """numpy in -> numpy (dA, dpi, dE)."""
    out = (fn or engine.posterior_grad_walk)(dev(A), dev(pi), dev(E), dev(G), mode=mode_of(log), eps=eps, **kw)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def held(got, ref_m, A, tag, assert_it=True):
    """One model under every norm; prints each figure, then asserts."""
    err, limit, off = pc.check(got, ref_m, A)
    for n in pc.NORMS:
        print("PGWSWEEP %s %s err %.3e limit %.3e e32 %.3e" % (tag, n, err[n], limit[n], ref_m["e32"][n]))
    print("PGWSWEEP %s off-support non-zeros %d" % (tag, off))
    if assert_it:
        assert all(np.isfinite(x).all() for x in got), tag
        bad = [(n, err[n], limit[n]) for n in limit if not err[n] <= limit[n]]
        assert not bad and off == 0, (tag, bad, off)


@pytest.mark.parametrize("spec", pc.all_specs(), ids=pc.spec_id)
def test_case_against_the_oracle(spec):
    c, refs = pc.build(spec), pc.reference(spec)
    got = run(c["A"], c["pi"], c["E"], c["G"], spec.log, spec.eps)
    k, q = len(spec.models), spec.q
    big = None
    if q <= 128:                                                               # the dense walk beside it: printed only
        big = run(c["A"], c["pi"], c["E"], c["G"], spec.log, spec.eps, fn=engine.posterior_grad_large)
    for m in range(k):
        tag = "%s m=%d" % (pc.spec_id(spec), m)
        if big is not None:
            held(pc.on_support([x[m] for x in big], c["A"][m]), refs[m], c["A"][m], tag + " (posterior_grad_large)", False)
        held([x[m] for x in got], refs[m], c["A"][m], tag)
        assert np.all(got[2][m][c["E"][m] <= spec.eps] == 0.0)
        assert np.all(got[1][m][c["pi"][m] <= spec.eps] == 0.0)
    if spec.L == 1:
        assert np.all(got[0] == 0.0)


def raw_call(A, pi, E, G, mode, outs, ws, eps=pc.EPS):
    k, b, L, q = E.shape
    rc = engine.lib().hmm_posterior_grad_walk(A.data_ptr(), pi.data_ptr(), E.data_ptr(), k, b, L, q, eps, mode,
                                              G.data_ptr(), *(t.data_ptr() for t in outs), ws.data_ptr(), ws.numel(),
                                              ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, rc
    torch.cuda.synchronize()


@pytest.mark.parametrize("log", pc.MODES)
def test_repeated_call_on_a_workspace_of_nan_bytes(log):
    spec = pc.batch_sweep()[4 + int(log)]                                      # gene + deg2, 127 states, b = 65
    assert (spec.b, spec.log, len(spec.models)) == (65, log, 2)
    c = pc.build(spec)
    A, pi, E, G = dev(c["A"]), dev(c["pi"]), dev(c["E"]), dev(c["G"])
    k, b, L, q = E.shape
    need = engine.lib().hmm_posterior_grad_walk_workspace_bytes(k, b, L, q)
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    outs = [torch.zeros((k, q, q), device=DEV), torch.zeros((k, q), device=DEV), torch.zeros_like(E)]
    raw_call(A, pi, E, G, mode_of(log), outs, ws)
    first = [t.clone() for t in outs]
    assert engine.lib().hmm_posterior_grad_walk_refused(k, b, L, q, ws.data_ptr(), need) == 0
    ws.fill_(0xFF)                                                             # every float a NaN
    for t in outs:
        t.fill_(float("nan"))
    raw_call(A, pi, E, G, mode_of(log), outs, ws)
    for x, y in zip(first, outs):
        assert torch.equal(x, y) and bool(torch.isfinite(y).all())
    assert engine.lib().hmm_posterior_grad_walk_refused(k, b, L, q, ws.data_ptr(), need) == 0


@pytest.mark.parametrize("log", pc.MODES)
def test_two_models_are_two_calls(log):
    spec = pc.length_sweep()[12 + int(log)]                                    # gene + deg1, 71 states, L = 17
    assert (spec.q, spec.L, spec.log, len(spec.models)) == (71, 17, log, 2)
    c = pc.build(spec)
    both = run(c["A"], c["pi"], c["E"], c["G"], log)
    for m in range(2):
        alone = run(*(c[n][m:m + 1] for n in ("A", "pi", "E", "G")), log)
        assert same([x[m:m + 1] for x in both], alone), m


@pytest.mark.parametrize("spec", pc.refused_cases(), ids=pc.spec_id)
def test_refused_model_next_to_a_served_one(spec):
    c, refs = pc.build(spec), pc.reference(spec)
    assert spec.models[0] == pc.REFUSED and refs[0] is None
    A, pi, E, G = c["A"], c["pi"], c["E"], c["G"]
    dims = E.shape
    got = run(A, pi, E, G, spec.log, check=False)
    assert engine.posterior_grad_walk_refused(dims) == 1
    alone = run(A[1:], pi[1:], E[1:], G[1:], spec.log)
    assert engine.posterior_grad_walk_refused((1,) + dims[1:]) == 0
    for x, y in zip(got, alone):
        assert np.isnan(x[0]).all()                                            # every output element of the refused model
        assert np.array_equal(x[1:], y)                                        # the served one: its own k = 1 call
    held([x[1] for x in got], refs[1], A[1], pc.spec_id(spec) + " m=1")
    with pytest.raises(engine.EngineError, match="refused"):
        engine.posterior_grad_walk(dev(A), dev(pi), dev(E), dev(G), mode=mode_of(spec.log), check=True)


def test_offsets_beyond_2_to_31():
    """k*b*L*q > 2^31 elements: many short sequences; three sampled sequences, the last included, against the oracle
    under the tensor norm of dE scaled by the sampled sequences' own maximum."""
    k, b, L, q = 1, 8192, 3700, 71
    assert k * b * L * q > 2 ** 31
    A, pi = five_copy()
    g = torch.Generator(device=DEV).manual_seed(9)
    E = torch.rand((k, b, L, q), generator=g, device=DEV) * 0.9 + 0.05
    G = -(torch.rand((k, b, L, q), generator=g, device=DEV) < 0.05).float()
    rows = [0, 4099, b - 1]
    want = pm.oracle(A, pi, E[0, rows].cpu().numpy(), G[0, rows].cpu().numpy(), True)[2]
    dA, dpi, dE = engine.posterior_grad_walk(dev(A[None]), dev(pi[None]), E, G, mode=engine.POST_LOG)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(dA).all()) and bool(torch.isfinite(dpi).all())
    assert bool(torch.isfinite(dE[0, -1]).all()) and bool(torch.isfinite(dE[0, :, -1]).all())
    assert bool((dA[0][dev(A) == 0] == 0).all())
    got = dE[0, rows].cpu().numpy()
    del dA, dpi, dE, E, G
    torch.cuda.empty_cache()
    err = np.abs(got - want).max((1, 2))
    print("PGWSWEEP offsets err", err, "scale", np.abs(want).max((1, 2)))
    assert np.all(err <= pm.TENSOR_REL * np.abs(want).max((1, 2)) + pm.TENSOR_ABS), err


def test_graph_capture_and_replay():
    spec = pc.gene_sweep()[7]                                                  # the nine-copy model, holes, log mode
    assert (spec.q, spec.emis, spec.log) == (127, "holes", True)
    c = pc.build(spec)
    A, pi = dev(c["A"]), dev(c["pi"])
    E, G = dev(c["E"][:, :, :50]), dev(c["G"][:, :, :50])
    E2, G2 = dev(np.ascontiguousarray(c["E"][:, :, 50:100])), dev(np.ascontiguousarray(c["G"][:, :, 50:100]))
    g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.stream(s):
        engine.posterior_grad_walk(A, pi, E, G)                                # (this stream's workspace)
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):                                    # one stream, no host synchronisation
            full = engine.posterior_grad_walk(A, pi, E, G, check=False)
        E.copy_(E2)                                                            # capture does not run the kernels
        G.copy_(G2)
        for t in full:
            t.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        want = engine.posterior_grad_walk(A, pi, E2, G2)
        torch.cuda.synchronize()
    for x, y in zip(full, want):
        assert torch.equal(x, y) and bool(torch.isfinite(y).all())


def posterior64(A, pi, E, eps, mode):
    """fp64 autograd through the cell's scaled forward and backward recursions with their clamps, one model: A (q,q),
    pi (q,), E (b,L,q) -> the posterior output of `mode` (b,L,q)."""
    L = E.shape[1]
    Ec = torch.clamp(E, min=eps)
    al, ll = [], 0.0
    a = Ec[:, 0] * torch.clamp(pi, min=eps)
    for t in range(L):
        if t:
            a = Ec[:, t] * torch.clamp(al[-1] @ A, min=eps)
        S = a.sum(-1, keepdim=True)
        ll = ll + torch.log(S)
        al.append(a / S)
    rb = [None] * L
    rb[L - 1] = torch.ones_like(al[0])
    for t in range(L - 2, -1, -1):
        sb = Ec[:, t + 1] * rb[t + 1]
        rb[t] = torch.clamp((sb / sb.sum(-1, keepdim=True)) @ A.T, min=eps)
    g = torch.stack(al, 1) * torch.stack(rb, 1)
    gamma = g / g.sum(-1, keepdim=True)
    if mode == engine.POST_PROB:
        return gamma
    return torch.log(gamma) + (ll[:, None] if mode == engine.POST_LOG_NO_LL else 0.0)


@pytest.mark.parametrize("mode", [engine.POST_PROB, engine.POST_LOG, engine.POST_LOG_NO_LL])
def test_autograd_support_only_against_fp64_cpu_autograd(mode):
    spec = pc.length_sweep()[12]._replace(models=("gene",))                    # 71 states, L = 17, dense G
    c = pc.build(spec)
    A, pi, E, G = c["A"], c["pi"], c["E"], c["G"]
    assert A.shape == (1, 71, 71)
    leaves = [dev(x).requires_grad_(True) for x in (A, pi, E)]
    out = autograd.posterior(*leaves, mode=mode, support_only="always")
    (out * dev(G)).sum().backward()
    torch.cuda.synchronize()
    ref = [torch.tensor(x[0], dtype=torch.float64, requires_grad=True) for x in (A, pi, E)]
    out64 = posterior64(*ref, pc.EPS, mode)
    (out64 * torch.tensor(G[0], dtype=torch.float64)).sum().backward()
    present = A[0] > 0
    got = [t.grad[0].cpu().numpy() for t in leaves]
    full = [t.grad.numpy() for t in ref]
    want = pc.on_support(full, A[0])
    assert np.all(got[0][~present] == 0.0) and np.abs(full[0][~present]).max() > 0          # dense autograd fills them
    for name, g, w in zip(("dA", "dpi", "dE"), got, want):
        err = np.abs(g - w).max()
        print("PGWSWEEP autograd mode %d %s err %.3e max|want| %.3e" % (mode, name, err, np.abs(w).max()))
        assert err <= pm.TENSOR_REL * np.abs(w).max() + pm.TENSOR_ABS, (name, err)
    fwd = out[0].detach().cpu().numpy()
    w64 = out64.detach().numpy()
    ok = np.isfinite(w64) & (w64 > -60 if mode != engine.POST_PROB else True)
    assert np.all(np.abs(fwd - w64)[ok] <= 1e-4 * np.abs(w64)[ok] + 2e-4)
    # the default leaves today's path untouched: its dA has the absent edges' derivatives
    plain = [dev(x).requires_grad_(True) for x in (A, pi, E)]
    (autograd.posterior(*plain, mode=mode) * dev(G)).sum().backward()
    assert float(plain[0].grad[0][torch.as_tensor(~present, device=DEV)].abs().max()) > 0


def test_support_only_is_ignored_at_seven_states():
    rng = np.random.default_rng(3)
    A7, pi7 = lc.gene7()
    E7 = lc.draw_E(rng, ("gene",), 2, 9, 7, "rare")
    G7 = rng.standard_normal(E7.shape).astype(np.float32)
    res = []
    for support in ("always", True, False):
        leaves = [dev(x).requires_grad_(True) for x in (A7[None], pi7[None], E7)]
        out = autograd.posterior(*leaves, support_only=support)
        (out * dev(G7)).sum().backward()
        res.append([out.detach()] + [t.grad for t in leaves])
    for r in res[:2]:
        assert all(torch.equal(x, y) for x, y in zip(r, res[2]))


def test_five_copy_layer_trains_through_the_posteriors_with_support_grad(monkeypatch):
    """loss.backward() through state_posterior_log_probs(x, training=True) of the 71-state layer with
    support_grad=True: forward through engine.posterior_walk and backward through engine.posterior_grad_walk where the
    predicates say 1 (they are tables of measurements: played here, 1 and 0), neither with 0; the transition kernel's
    gradient agrees between the two within the tolerance of test_five_copy_layer_with_support_grad."""
    from hmm_layer_amd.MsaHmmCell import HmmCell
    from hmm_layer_amd.MsaHMMLayer import MsaHmmLayer
    from hmm_layer_amd.gene_pred_hmm_emitter import GenePredHMMEmitter
    from hmm_layer_amd.gene_pred_hmm_transitioner import GenePredMultiHMMTransitioner
    b, L = 2, 160
    g = torch.Generator().manual_seed(13)
    cls = torch.softmax(2 * torch.randn((1, b, L, 15), generator=g), -1)
    nuc = torch.nn.functional.one_hot(torch.randint(0, 4, (1, b, L), generator=g), 5).float()
    x = torch.cat([cls, nuc], -1).to(DEV)
    labels = torch.nn.functional.one_hot(torch.randint(0, 71, (b, L), generator=g), 71).float().to(DEV)
    calls = []
    for name in ("posterior_walk", "posterior_grad_walk"):
        def spy(*a, _real=getattr(engine, name), _name=name, **kw):
            calls.append(_name)
            return _real(*a, **kw)
        monkeypatch.setattr(engine, name, spy)
    grads = {}
    for pays in (1, 0):
        for pred in ("hmm_posterior_grad_walk_pays", "hmm_loglik_grad_walk_pays"):
            monkeypatch.setattr(engine.lib(), pred, lambda *dims, _v=pays: _v)
        torch.manual_seed(5)
        np.random.seed(5)
        em = GenePredHMMEmitter(**CODONS, num_copies=5)
        em.build((1, b, L, 15))
        tr = GenePredMultiHMMTransitioner(k=5, initial_exon_len=200, initial_intron_len=4500, initial_ir_len=10000,
                                          support_grad=True)
        cell = HmmCell([71], 15, em, tr).to(DEV)
        layer = MsaHmmLayer(cell, use_prior=False)
        layer.build(x.shape)
        del calls[:]
        post = layer.state_posterior_log_probs(x, training=True)
        assert calls == (["posterior_walk"] if pays else []), (pays, calls)
        loss = -(labels * post.reshape(labels.shape)).mean()
        loss.backward()
        assert calls == (["posterior_walk", "posterior_grad_walk"] if pays else []), (pays, calls)
        gk = cell.transitioner.transition_kernel.grad
        assert gk is not None and bool(torch.isfinite(gk).all()) and float(gk.abs().max()) > 0
        grads[pays] = gk.clone()
    want = grads[0]
    err = float((grads[1] - want).abs().max())
    print("PGWSWEEP layer err %.3e max|want| %.3e" % (err, float(want.abs().max())))
    assert err <= 5e-4 * float(want.abs().max()) + 1e-7
