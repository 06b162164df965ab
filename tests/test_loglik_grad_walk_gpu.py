"""hmm_loglik_grad_walk (engine.loglik_grad_walk, 65..256 states, the per-sequence walk with the sparse step) on the
device: every case of tests/loglik_grad_walk_cases.py against the fp64 Baum-Welch oracle under the project's norms
(that module's docstring; nothing in a limit comes from engine output), exact zeros in dA wherever A == 0, and the
properties the header promises: the log-likelihood form bit-identical to the gradient call's loglik, grad_loglik = NULL
bit-identical to ones, k = 2 bit-identical to two k = 1 calls, a repeated call on a dirtied workspace and dirtied
outputs bit-identical, agreement with hmm_loglik_grad_large's walk where that serves (65..128 states), the refusal of a
model outside the sparse rule next to a served one, one offset beyond 2^31 elements, graph capture of both forms, the
autograd node and the five-copy layer."""
import ctypes

import numpy as np
import pytest
import torch

from hmm_layer_amd import autograd, engine
from oracle import ref_cell, textbook

import loglik_grad_walk_cases as wc
from test_loglik_grad_large_gpu import CODONS, five_copy

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(x):
    return torch.as_tensor(np.asarray(x), dtype=torch.float32, device=DEV)


def run(A, pi, E, w=None, eps=wc.EPS, **kw):
    """numpy in -> numpy (dA, dpi, dE, ll) (None where not asked for)."""
    out = engine.loglik_grad_walk(dev(A), dev(pi), dev(E), None if w is None else dev(w), eps=eps, **kw)
    torch.cuda.synchronize()
    return [None if t is None else t.cpu().numpy() for t in out]


def same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def held(got, ref_m, A, tag):
    """One model under every norm; prints each figure, then asserts."""
    err, limit, off = wc.check(got, ref_m, A)
    for n in wc.TENSOR_NORMS + wc.FINE_NORMS:
        print("GWSWEEP %s %s err %.3e limit %.3e" % (tag, n, err[n], limit[n]))
    print("GWSWEEP %s off-support non-zeros %d" % (tag, off))
    assert all(np.isfinite(x).all() for x in got), tag
    bad = [(n, err[n], limit[n]) for n in limit if not err[n] <= limit[n]]
    assert not bad and off == 0, (tag, bad, off)


@pytest.mark.parametrize("spec", wc.all_specs(), ids=wc.spec_id)
def test_case_against_the_oracle(spec):
    c, refs = wc.build(spec), wc.reference(spec)
    got = run(c["A"], c["pi"], c["E"], c["w"], spec.eps)
    k, q = len(spec.models), spec.q
    for m in range(k):
        held([x[m] for x in got], refs[m], c["A"][m], "%s m=%d" % (wc.spec_id(spec), m))
        assert np.all(got[2][m][c["E"][m] <= spec.eps] == 0.0)                 # position 0 included, after dpi
        if c["w"] is not None:
            assert np.all(got[2][m][c["w"][m] == 0] == 0.0)
    if spec.L == 1:
        assert np.all(got[0] == 0.0)
    # the log-likelihood form: the same bits, and no gradient
    only = run(c["A"], c["pi"], c["E"], None, spec.eps, want_grads=False)
    assert only[:3] == [None, None, None] and np.array_equal(only[3], got[3])
    # where hmm_loglik_grad_large's walk serves: the same derivative on present edges, dpi, dE and ll, the same norms
    if q <= 128:
        with engine.option(engine.OPT_GLARGE, 1):
            big = engine.loglik_grad_large(dev(c["A"]), dev(c["pi"]), dev(c["E"]),
                                           None if c["w"] is None else dev(c["w"]), eps=spec.eps)
            torch.cuda.synchronize()
        big = [t.cpu().numpy() for t in big]
        for m in range(k):
            stand_in = dict(refs[m], want=tuple(np.asarray(x[m], np.float64) for x in big))
            err, limit, _ = wc.check([x[m] for x in got], stand_in, c["A"][m])
            bad = [(n, err[n], limit[n]) for n in limit if not err[n] <= limit[n]]
            assert not bad, (wc.spec_id(spec), m, bad)


def test_no_weights_is_ones_and_two_models_are_two_calls():
    spec = wc.length_sweep()[6]                                                # gene + deg1, 71 states, L = 17
    assert (spec.q, spec.L, len(spec.models)) == (71, 17, 2)
    c = wc.build(spec)
    A, pi, E = c["A"], c["pi"], c["E"]
    none, ones = run(A, pi, E, None), run(A, pi, E, np.ones(E.shape[:2], np.float32))
    assert same(none, ones)
    both = run(A, pi, E, c["w"])
    for m in range(2):
        alone = run(A[m:m + 1], pi[m:m + 1], E[m:m + 1], c["w"][m:m + 1])
        assert same([x[m:m + 1] for x in both], alone), m


def raw_call(A, pi, E, w, outs, ws, eps=wc.EPS):
    k, b, L, q = E.shape
    rc = engine.lib().hmm_loglik_grad_walk(A.data_ptr(), pi.data_ptr(), E.data_ptr(), k, b, L, q, eps,
                                           None if w is None else w.data_ptr(),
                                           *(None if t is None else t.data_ptr() for t in outs), ws.data_ptr(),
                                           ws.numel(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, rc
    torch.cuda.synchronize()


@pytest.mark.parametrize("grads", [True, False])
def test_repeated_call_on_dirtied_workspace_and_outputs(grads):
    spec = wc.batch_sweep()[2]                                                 # gene + deg2, 127 states, b = 65
    c = wc.build(spec)
    A, pi, E, w = dev(c["A"]), dev(c["pi"]), dev(c["E"]), dev(c["w"])
    k, b, L, q = E.shape
    need = engine.lib().hmm_loglik_grad_walk_workspace_bytes(k, b, L, q)
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    outs = [torch.zeros((k, q, q), device=DEV), torch.zeros((k, q), device=DEV), torch.zeros_like(E)] if grads \
        else [None, None, None]
    outs.append(torch.zeros((k, b), dtype=torch.float64, device=DEV))
    raw_call(A, pi, E, w if grads else None, outs, ws)
    first = [None if t is None else t.clone() for t in outs]
    assert engine.lib().hmm_loglik_grad_walk_refused(k, b, L, q, ws.data_ptr(), need) == 0
    ws.fill_(0xAB)
    for t in outs:
        if t is not None:
            t.fill_(float("nan"))
    raw_call(A, pi, E, w if grads else None, outs, ws)
    for x, y in zip(first, outs):
        assert (x is None and y is None) or torch.equal(x, y)
    assert bool(torch.isfinite(outs[3]).all())
    assert engine.lib().hmm_loglik_grad_walk_refused(k, b, L, q, ws.data_ptr(), need) == 0


def test_refused_model_next_to_a_served_one():
    spec = wc.refused_case()
    c, refs = wc.build(spec), wc.reference(spec)
    assert spec.models[0] == wc.REFUSED and refs[0] is None
    A, pi, E, w = c["A"], c["pi"], c["E"], c["w"]
    dims = E.shape
    for want_grads in (True, False):
        got = run(A, pi, E, w if want_grads else None, check=False, want_grads=want_grads)
        assert engine.loglik_grad_walk_refused(dims) == 1
        alone = run(A[1:], pi[1:], E[1:], w[1:] if want_grads else None, want_grads=want_grads)
        assert engine.loglik_grad_walk_refused((1,) + dims[1:]) == 0
        for x, y in zip(got, alone):
            if x is not None:
                assert np.isnan(x[0]).all()                                    # every output element of the refused model
                assert np.array_equal(x[1:], y)                                # the served one: its own k = 1 call
        if want_grads:
            held([x[1] for x in got], refs[1], A[1], "refused-case m=1")
        with pytest.raises(engine.EngineError, match="refused"):
            engine.loglik_grad_walk(dev(A), dev(pi), dev(E), want_grads=want_grads, check=True)
    with pytest.raises(engine.EngineError, match="refused"):                   # the node checks in its forward
        autograd.loglik(dev(A), dev(pi), dev(E), support_only="always")


def test_offsets_beyond_2_to_31():
    """k*b*L*q > 2^31 elements (dE beyond 8 GB), as tests/test_loglik_grad_large_gpu.py builds it: sampled sequences,
    the last included."""
    k, b, L, q = 1, 1024, 30000, 71
    assert k * b * L * q > 2 ** 31
    A, pi = five_copy()
    g = torch.Generator(device=DEV).manual_seed(9)
    E = torch.rand((k, b, L, q), generator=g, device=DEV) * 0.9 + 0.05
    rows = [0, 517, b - 1]
    Es = E[0, rows].cpu().numpy()
    rE = textbook.loglik_grad(A, pi, Es)[2]
    ll64 = textbook.loglik(A, pi, Es)
    dA, dpi, dE, ll = engine.loglik_grad_walk(dev(A[None]), dev(pi[None]), E)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(dA).all()) and bool(torch.isfinite(dpi).all())
    assert bool(torch.isfinite(dE[0, -1]).all()) and bool(torch.isfinite(dE[0, :, -1]).all())
    assert bool((dA[0][dev(A) == 0] == 0).all())
    got = dE[0, rows].cpu().numpy()
    assert np.all(np.abs(got - rE) <= 2e-5 * np.abs(rE).max() + 1e-4 * np.abs(rE)), np.abs(got - rE).max()
    llr = ll[0, rows].cpu().numpy()
    assert np.all(np.abs(llr - ll64) <= 1e-6 * np.abs(ll64) + 2e-4)
    del dA, dpi, dE
    only = engine.loglik_grad_walk(dev(A[None]), dev(pi[None]), E, want_grads=False)[3]
    assert torch.equal(only, ll)
    del E
    torch.cuda.empty_cache()


def test_graph_capture_and_replay_of_both_forms():
    spec = wc.gene_sweep()[3]                                                  # the nine-copy model, holes
    assert spec.q == 127
    c = wc.build(spec)
    A, pi, w = dev(c["A"]), dev(c["pi"]), dev(c["w"])
    E = dev(c["E"][:, :, :50])
    E2 = dev(np.ascontiguousarray(c["E"][:, :, 50:100]))
    g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.stream(s):
        engine.loglik_grad_walk(A, pi, E, w)                                   # (this stream's workspace)
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):                                    # one stream, no host synchronisation
            full = engine.loglik_grad_walk(A, pi, E, w, check=False)
            only = engine.loglik_grad_walk(A, pi, E, want_grads=False, check=False)
        E.copy_(E2)                                                            # capture does not run the kernels
        for t in full + (only[3],):
            t.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        want = engine.loglik_grad_walk(A, pi, E2, w)
        torch.cuda.synchronize()
    for x, y in zip(full, want):
        assert torch.equal(x, y)
    assert torch.equal(only[3], want[3]) and bool(torch.isfinite(want[0]).all())


def loglik64(A, pi, E, eps):
    """fp64 autograd through the cell's scaled forward recursion with its clamps, one model: A (q,q), pi (q,),
    E (b,L,q) -> loglik (b,)."""
    a = torch.clamp(E[:, 0], min=eps) * torch.clamp(pi, min=eps)
    S = a.sum(-1, keepdim=True)
    ll, a = torch.log(S), a / S
    for t in range(1, E.shape[1]):
        a = torch.clamp(E[:, t], min=eps) * torch.clamp(a @ A, min=eps)
        S = a.sum(-1, keepdim=True)
        ll, a = ll + torch.log(S), a / S
    return ll[:, 0]


def test_autograd_support_only_against_fp64_cpu_autograd():
    spec = wc.length_sweep()[6]._replace(models=("gene",))
    c = wc.build(spec)
    A, pi, E, w = c["A"], c["pi"], c["E"], c["w"]
    assert A.shape == (1, 71, 71)
    leaves = [dev(x).requires_grad_(True) for x in (A, pi, E)]
    ll = autograd.loglik(*leaves, support_only="always")
    (ll * dev(w).double()).sum().backward()
    torch.cuda.synchronize()
    ref = [torch.tensor(x[0], dtype=torch.float64, requires_grad=True) for x in (A, pi, E)]
    ll64 = loglik64(*ref, wc.EPS)
    (ll64 * torch.tensor(w[0], dtype=torch.float64)).sum().backward()
    got = [t.grad[0].cpu().numpy() for t in leaves] + [ll[0].detach().cpu().numpy()]
    want = [t.grad.numpy() for t in ref] + [ll64.detach().numpy()]
    present = A[0] > 0
    assert np.all(got[0][~present] == 0.0) and np.abs(want[0][~present]).max() > 0          # dense autograd fills them
    assert np.abs(got[0] - want[0])[present].max() <= 2e-4 * np.abs(want[0]).max()
    assert np.abs(got[1] - want[1]).max() <= 2e-4 * np.abs(want[1]).max()
    assert np.all(np.abs(got[2] - want[2]) <= 2e-5 * np.abs(want[2]).max() + 1e-4 * np.abs(want[2]))
    assert np.all(np.abs(got[3] - want[3]) <= 1e-6 * np.abs(want[3]) + 2e-4)
    # the default leaves today's path untouched: its dA has the absent edges' derivatives
    plain = [dev(x).requires_grad_(True) for x in (A, pi, E)]
    (autograd.loglik(*plain) * dev(w).double()).sum().backward()
    assert float(plain[0].grad[0][torch.as_tensor(~present, device=DEV)].abs().max()) > 0
    # outside 65..256 states the argument is ignored
    rng = np.random.default_rng(3)
    A7, pi7 = wc.lc.gene7()
    E7 = dev(wc.draw_E(rng, ("gene",), 2, 9, 7, "rare"))
    a = autograd.loglik(dev(A7[None]), dev(pi7[None]), E7, support_only="always")
    assert torch.equal(a, autograd.loglik(dev(A7[None]), dev(pi7[None]), E7))


def test_five_copy_layer_with_support_grad(monkeypatch):
    """loss.backward() through the 71-state layer with support_grad=True: both sweeps go through
    engine.loglik_grad_walk where the predicate says 1 (it is a table of measurements: played here, 1 and 0), and the
    transition kernel's gradient is held to the tolerances of test_five_copy_gene_model_is_trainable."""
    from hmm_layer_amd.MsaHmmCell import HmmCell
    from hmm_layer_amd.MsaHMMLayer import MsaHmmLayer
    from hmm_layer_amd.gene_pred_hmm_emitter import GenePredHMMEmitter
    from hmm_layer_amd.gene_pred_hmm_transitioner import GenePredMultiHMMTransitioner
    b, L = 2, 160
    g = torch.Generator().manual_seed(13)
    cls = torch.softmax(2 * torch.randn((1, b, L, 15), generator=g), -1)
    nuc = torch.nn.functional.one_hot(torch.randint(0, 4, (1, b, L), generator=g), 5).float()
    x = torch.cat([cls, nuc], -1).to(DEV)
    calls = []
    real = engine.loglik_grad_walk

    def spy(*a, **kw):
        calls.append((kw.get("want_grads", True), kw.get("check", True)))
        return real(*a, **kw)

    monkeypatch.setattr(engine, "loglik_grad_walk", spy)
    grads = {}
    for pays in (1, 0):
        monkeypatch.setattr(engine.lib(), "hmm_loglik_grad_walk_pays", lambda *dims, _v=pays: _v)
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
        loglik, mean = layer(x, training=True)
        (-mean).backward()
        assert calls == ([(False, True), (True, False)] if pays else []), (pays, calls)
        gk = cell.transitioner.transition_kernel.grad
        assert gk is not None and bool(torch.isfinite(gk).all()) and float(gk.abs().max()) > 0
        grads[pays] = gk.clone()
        if not pays:
            continue
        cell.recurrent_init()
        E = cell.emission_probs(x, end_hints=None, training=True).to(torch.float32)
        A, pi = cell.A, cell.init_dist.reshape(1, 71)
        gl = torch.full((1, b), -1.0 / b)
        dA, dpi, dE, ll_ref = ref_cell.loglik_grad(A.detach().cpu(), pi.detach().cpu(), E.detach().cpu(), gl)
        want = torch.autograd.grad([A, E], [cell.transitioner.transition_kernel], [dA.to(DEV), dE.to(DEV)])[0]
        assert float((gk - want).abs().max()) <= 5e-4 * float(want.abs().max()) + 1e-7
        assert np.abs(loglik.detach().cpu().numpy() - ll_ref.numpy()).max() <= 2e-3
    # the same model on today's path: the parameters' gradients agree (the mask proof of the CPU test, in fp32)
    assert float((grads[1] - grads[0]).abs().max()) <= 5e-4 * float(grads[0].abs().max()) + 1e-7
