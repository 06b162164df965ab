"""hmm_class_posterior / hmm_class_posterior_grad (engine.class_posterior, engine.class_posterior_grad; up to 16 states)
on the device.

Forward: out_prob bit for bit the sequential fp32 class sums of engine.posterior(POST_PROB)'s gamma (numpy, increasing
state index from 0.0f), the bits hmm_posterior_decode compares, hmm_posterior's log-likelihood, out_log within 2 ulp of
the fp64 log of out_prob, and the fp64 oracle's class sums within the tolerance of tests/test_posterior_decode_gpu.py
(n_max * 2e-5).  Backward: every case of tests/class_posterior_cases.py against the fp64 oracle under the project's four
norms (nothing in a limit comes from engine output); prob mode bit for bit engine.posterior_grad(POST_PROB) on the
expanded gradient, log mode the same on Gc / P expanded (the quotient in numpy fp32), under HMM_OPT_PGCHUNK = 2 and 0 so
that both sweeps are compared under identical routing; the serial count against the predicted verdicts.  And the
properties the header promises for both calls."""
import ctypes

import numpy as np
import pytest
import torch

from hmm_layer_amd import autograd, engine
from hmm_layer_amd.MsaHMMLayer import MsaHmmLayer

import class_posterior_cases as cc
import class_posterior_walk_cases as cw
import posterior_decode_mid_cases as dm
import postgrad_small_cases as ps
from test_layer_gpu import gene_setup

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ALL = cc.all_specs()
FWD_SPECS = [s for s in ALL if not s.log]                    # (the mode does not enter the forward)


def dev(x):
    return torch.as_tensor(np.asarray(x), dtype=torch.float32, device=DEV)


def mode_of(log):
    return engine.POST_LOG if log else engine.POST_PROB


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def ctable(table):
    return (ctypes.c_int * len(table))(*table)


def forward(c, spec, prob=True, log=True):
    table, C = cc.table_of(spec)
    out = engine.class_posterior(dev(c["A"]), dev(c["pi"]), dev(c["E"]), list(table), C, eps=spec.eps, prob=prob, log=log)
    torch.cuda.synchronize()
    return [None if t is None else t.cpu().numpy() for t in out]


def backward(A, pi, E, G, P, table, C, log, eps=cc.EPS):
    out = engine.class_posterior_grad(dev(A), dev(pi), dev(E), list(table), C, dev(G),
                                      class_prob=None if P is None else dev(P), mode=mode_of(log), eps=eps)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def state_backward(A, pi, E, G, eps=cc.EPS):
    out = engine.posterior_grad(dev(A), dev(pi), dev(E), dev(G), mode=engine.POST_PROB, eps=eps)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def quotient(G, P):
    """G' of the header in numpy fp32: the IEEE quotient, 0 where the class posterior is 0."""
    G, P = np.asarray(G, np.float32), np.asarray(P, np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(P > 0, G / P, np.float32(0)).astype(np.float32)


def sequential_sums(gamma, table, C):
    """The class sums as the kernel forms them: fp32, states in increasing index, from 0.0f, one rounding per state."""
    out = np.zeros(gamma.shape[:-1] + (C,), np.float32)
    for s, cl in enumerate(table):
        out[..., cl] = out[..., cl] + gamma[..., s]
    return out


def same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def check_log(P, Lg, tag):
    zero = P == 0
    assert np.all(np.isneginf(Lg[zero])) and np.all(np.isfinite(Lg[~zero])), tag
    want = np.log(P[~zero].astype(np.float64))
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    worst = float((np.abs(Lg[~zero] - want) / ulp).max()) if want.size else 0.0
    print("CPSWEEP %s log: %.2f ulp" % (tag, worst))
    assert worst <= 2.0, (tag, worst)


@pytest.mark.parametrize("spec", FWD_SPECS, ids=cc.spec_id)
def test_forward(spec):
    c, refs = cc.build(spec), cc.reference(spec)
    table, C = cc.table_of(spec)
    tag = cc.spec_id(spec)
    A, pi, E = dev(c["A"]), dev(c["pi"]), dev(c["E"])
    with engine.option(engine.OPT_CHUNK, spec.T):
        P, Lg, ll = forward(c, spec)
        gamma, ll_post = engine.posterior(A, pi, E, mode=engine.POST_PROB, eps=spec.eps)
        label, conf, ll_dec = engine.posterior_decode(A, pi, E, state_class=list(table), num_classes=C, eps=spec.eps)
        only_p, only_l = forward(c, spec, log=False)[0], forward(c, spec, prob=False)[1]
    gamma = gamma.cpu().numpy()
    # the sequential fp32 sums of hmm_posterior's gamma, bit for bit; with the table range(q) that gamma itself
    assert np.array_equal(P, sequential_sums(gamma, table, C)), tag
    if spec.table == "id":
        assert np.array_equal(P, gamma)
    # the bits hmm_posterior_decode compares, and hmm_posterior's log-likelihood
    label = label.cpu().numpy()
    assert np.array_equal(np.take_along_axis(P, label[..., None].astype(np.int64), -1)[..., 0], conf.cpu().numpy()), tag
    assert np.array_equal(P.argmax(-1), label), tag                             # (numpy: the first maximal index)
    assert np.array_equal(ll, ll_post.cpu().numpy()) and np.array_equal(ll, ll_dec.cpu().numpy()), tag
    # one output or both: the same bits
    assert np.array_equal(only_p, P) and np.array_equal(only_l, Lg, equal_nan=True), tag
    check_log(P, Lg, tag)
    used = np.bincount(np.asarray(table), minlength=C) > 0
    assert np.all(P[..., ~used] == 0) and np.all(np.isneginf(Lg[..., ~used]))   # an empty class: exactly 0 and -inf
    # the fp64 oracle's class sums
    n = dm.largest_class(table, C)
    for m, ref in enumerate(refs):
        err = float(np.abs(P[m] - ref["P"]).max())
        print("CPSWEEP %s m=%d oracle: err %.3e bound %.3e" % (tag, m, err, n * dm.STATE_TOL))
        assert err <= n * dm.STATE_TOL, (tag, m, err)


def test_forward_in_the_windows_and_whole_sequence_kernels():
    """The stretch case: one sequence leaves the scan plan (windows or whole); and everything whole under
    HMM_EXACT_ALWAYS.  The class sums are those of hmm_posterior's gamma in either kernel, bit for bit."""
    spec = [s for s in FWD_SPECS if s.emis == "stretch"][0]
    c = cc.build(spec)
    table, C = cc.table_of(spec)
    A, pi, E = dev(c["A"]), dev(c["pi"]), dev(c["E"])
    dims = tuple(E.shape)
    with engine.option(engine.OPT_CHUNK, spec.T):
        P = forward(c, spec)[0]
        routed = engine.exact_count(engine.OP_POSTERIOR, dims, tag=engine.CLASS_TAG)
        detail = engine.exact_detail(dims, tag=engine.CLASS_TAG)
        gamma = engine.posterior(A, pi, E, eps=spec.eps)[0].cpu().numpy()
        assert routed == engine.exact_count(engine.OP_POSTERIOR, dims) >= 1
        print("CPSWEEP stretch routing", detail)
        assert np.array_equal(P, sequential_sums(gamma, table, C))
        with engine.option(engine.OPT_EXACT, engine.EXACT_ALWAYS):
            Pw, Lw, llw = forward(c, spec)
            assert engine.exact_count(engine.OP_POSTERIOR, dims, tag=engine.CLASS_TAG) == dims[0] * dims[1]
            gw, ll = engine.posterior(A, pi, E, eps=spec.eps)
            assert np.array_equal(Pw, sequential_sums(gw.cpu().numpy(), table, C))
            assert np.array_equal(llw, ll.cpu().numpy())
            check_log(Pw, Lw, "exact-always")


def held(got, ref_m, A, name, per_chunk, tag):
    err, limit = cc.check(got, ref_m, A, name, per_chunk)
    for n in limit:
        print("CPSWEEP %s %s err %.3e limit %.3e" % (tag, n, err[n], limit[n]))
    assert all(np.isfinite(x).all() for x in got), tag
    bad = [(n, err[n], limit[n]) for n in limit if not err[n] <= limit[n]]
    if ref_m["absolute"] is not None:
        worst = [float(np.abs(x).max()) for x in got]
        print("CPSWEEP %s absolute %s bound %s" % (tag, worst, ref_m["absolute"]))
        bad += [("absolute", w, a) for w, a in zip(worst, ref_m["absolute"]) if not w <= a]
    assert not bad, (tag, bad)


@pytest.mark.parametrize("spec", ALL, ids=cc.spec_id)
def test_backward(spec):
    c, refs = cc.build(spec), cc.reference(spec)
    table, C = cc.table_of(spec)
    tag = cc.spec_id(spec)
    A, pi, E, G = c["A"], c["pi"], c["E"], c["G"]
    dims = E.shape
    n = dims[0] * dims[1]
    with engine.option(engine.OPT_CHUNK, spec.T):
        P = forward(c, spec, log=False)[0]
        Gs = cc.expand(quotient(G, P) if spec.log else G, table)
        got = backward(A, pi, E, G, P if spec.log else None, table, C, spec.log, spec.eps)
        serial = engine.class_posterior_grad_serial_count(dims)
        lo, hi = cc.serial_bounds(spec)
        print("CPSWEEP %s serial %d of %d predicted %d..%d" % (tag, serial, n, lo, hi))
        assert lo <= serial <= hi, (tag, serial, lo, hi)
        if not spec.log:                                                        # the same routing rules: bit for bit
            assert same(got, state_backward(A, pi, E, Gs, spec.eps)), tag
        for force in (2, 0):                                                    # identical routing for both calls
            if force == 2 and not cc.forced_per_chunk(spec):
                continue
            with engine.option(engine.OPT_PGCHUNK, force):
                mine = backward(A, pi, E, G, P if spec.log else None, table, C, spec.log, spec.eps)
                assert same(mine, state_backward(A, pi, E, Gs, spec.eps)), (tag, force)
    if spec.q == 1:
        assert all(np.all(x == 0.0) for x in got)                               # exact zeros
    per_chunk = cc.shipped_per_chunk(spec) and serial < n
    for m, name in enumerate(spec.models):
        held([x[m] for x in got], refs[m], A[m], name, per_chunk, "%s m=%d" % (tag, m))
        assert np.all(got[2][m][E[m] <= spec.eps] == 0.0)


def dead_class_inputs():
    """Five states of which the last is never entered, never left, never started in and never emitted: its posterior
    underflows to exactly 0 in fp32 before the last position.  It is a class of its own."""
    rng = np.random.default_rng(44)
    q, b, L = 5, 3, 40
    A = rng.random((1, q, q)).astype(np.float32) + 0.1
    A[0, :, 4] = 0.0
    A[0, 4, :] = 0.0
    A[0, :4] /= A[0, :4].sum(-1, keepdims=True)
    pi = np.array([[0.25, 0.25, 0.25, 0.25, 0.0]], np.float32)
    E = (rng.random((1, b, L, q)) * 0.9 + 0.05).astype(np.float32)
    E[..., 4] = 0.0
    return A, pi, E, [0, 0, 1, 1, 2], 3


@pytest.mark.parametrize("log", cc.MODES)
def test_a_class_of_posterior_zero_passes_nothing(log):
    A, pi, E, table, C = dead_class_inputs()
    P, Lg, _ = engine.class_posterior(dev(A), dev(pi), dev(E), table, C, log=True)
    P, Lg = P.cpu().numpy(), Lg.cpu().numpy()
    dead = P[..., 2] == 0
    assert dead[..., :-1].all()                                                 # the class is not empty; its posterior is 0
    assert np.all(np.isneginf(Lg[..., 2][dead])) and np.isfinite(Lg[..., :2]).all()
    G = np.random.default_rng(5).standard_normal(P.shape).astype(np.float32)
    got = backward(A, pi, E, G, P, table, C, log)
    assert all(np.isfinite(x).all() for x in got)
    if log:                                                                     # G' = 0 there: the same call without it
        G2 = G.copy()
        G2[..., 2][dead] = 0.0
        assert same(got, backward(A, pi, E, G2, P, table, C, log))
        Gs = cc.expand(quotient(G, P), table)
        with engine.option(engine.OPT_PGCHUNK, 0):
            assert same(backward(A, pi, E, G, P, table, C, log), state_backward(A, pi, E, Gs))


def raw_forward(A, pi, E, ctab, C, P, Lg, ll, ws, eps=cc.EPS):
    k, b, L, q = E.shape
    rc = engine.lib().hmm_class_posterior(A.data_ptr(), pi.data_ptr(), E.data_ptr(), k, b, L, q, eps, ctab, C,
                                          P.data_ptr(), Lg.data_ptr(), ll.data_ptr(), ws.data_ptr(), ws.numel(), stream())
    assert rc == 0, rc


def raw_backward(A, pi, E, mode, ctab, C, P, G, outs, ws, eps=cc.EPS):
    k, b, L, q = E.shape
    rc = engine.lib().hmm_class_posterior_grad(A.data_ptr(), pi.data_ptr(), E.data_ptr(), k, b, L, q, eps, mode, ctab, C,
                                               P.data_ptr(), G.data_ptr(), *(t.data_ptr() for t in outs), ws.data_ptr(),
                                               ws.numel(), stream())
    assert rc == 0, rc


def buffers(E, C):
    k, b, L, q = E.shape
    lib = engine.lib()
    wf = torch.zeros(lib.hmm_class_posterior_workspace_bytes(k, b, L, q), dtype=torch.uint8, device=DEV)
    wb = torch.zeros(lib.hmm_class_posterior_grad_workspace_bytes(k, b, L, q, C), dtype=torch.uint8, device=DEV)
    fwd = [torch.zeros((k, b, L, C), device=DEV), torch.zeros((k, b, L, C), device=DEV),
           torch.zeros((k, b), dtype=torch.float64, device=DEV)]
    outs = [torch.zeros((k, q, q), device=DEV), torch.zeros((k, q), device=DEV), torch.zeros_like(E)]
    return wf, wb, fwd, outs


def two_model_case(log):
    spec = [s for s in cc.model_cases() if s.models == ("gene", "shipped") and s.log == log][0]
    return spec, cc.build(spec), cc.table_of(spec)


@pytest.mark.parametrize("log", cc.MODES)
def test_repeated_calls_on_workspaces_of_nan_bytes(log):
    spec, c, (table, C) = two_model_case(log)                                   # k = 2, one model routed per model
    ctab = ctable(table)
    A, pi, E, G = dev(c["A"]), dev(c["pi"]), dev(c["E"]), dev(c["G"])
    with engine.option(engine.OPT_CHUNK, spec.T):
        wf, wb, fwd, outs = buffers(E, C)
        raw_forward(A, pi, E, ctab, C, *fwd, wf)
        raw_backward(A, pi, E, mode_of(log), ctab, C, fwd[0], G, outs, wb)
        torch.cuda.synchronize()
        first = [t.clone() for t in fwd + outs]
        P = fwd[0].clone()
        for ws in (wf, wb):
            ws.fill_(0xFF)                                                     # every float a NaN
        for t in fwd + outs:
            t.fill_(float("nan"))
        raw_forward(A, pi, E, ctab, C, *fwd, wf)
        raw_backward(A, pi, E, mode_of(log), ctab, C, P, G, outs, wb)
        torch.cuda.synchronize()
    for x, y in zip(first, fwd + outs):
        assert torch.equal(x, y)
    assert all(bool(torch.isfinite(y).all()) for y in [fwd[0], fwd[2]] + outs)


def test_graph_capture_and_replay_keeps_the_table():
    spec = [s for s in cc.geometry_sweep() if s.q == 15 and s.L == 100 and s.T == 16 and s.log][0]
    c = cc.build(spec)
    table, C = cc.table_of(spec)
    ctab = ctable(table)
    A, pi = dev(c["A"]), dev(c["pi"])
    E, G = dev(c["E"][:, :, :50]), dev(c["G"][:, :, :50])
    E2, G2 = dev(np.ascontiguousarray(c["E"][:, :, 50:])), dev(np.ascontiguousarray(c["G"][:, :, 50:]))
    with engine.option(engine.OPT_CHUNK, 16):
        wf, wb, fwd, outs = buffers(E, C)
        g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
        with torch.cuda.stream(s):
            raw_forward(A, pi, E, ctab, C, *fwd, wf)                           # (loads the kernels before the capture)
            raw_backward(A, pi, E, engine.POST_LOG, ctab, C, fwd[0], G, outs, wb)
            torch.cuda.synchronize()
            with torch.cuda.graph(g, stream=s):                                # one stream, no host synchronisation
                raw_forward(A, pi, E, ctab, C, *fwd, wf)
                raw_backward(A, pi, E, engine.POST_LOG, ctab, C, fwd[0], G, outs, wb)
            for i in range(len(table)):                                        # the host table: read at capture, by value
                ctab[i] = 0
            E.copy_(E2)                                                        # capture does not run the kernels
            G.copy_(G2)
            for t in fwd + outs:
                t.fill_(float("nan"))
            g.replay()
            torch.cuda.synchronize()
            wantf = engine.class_posterior(A, pi, E2, list(table), C, log=True)
            wantb = engine.class_posterior_grad(A, pi, E2, list(table), C, G2, class_prob=wantf[0])
            torch.cuda.synchronize()
    for x, y in zip(fwd + outs, list(wantf) + list(wantb)):
        assert torch.equal(x, y)
    assert all(bool(torch.isfinite(y).all()) for y in [fwd[0], fwd[2]] + outs)


def test_class_outputs_beyond_2_to_31_elements():
    """q = 2, C = 16: the class tensors pass 2^31 elements while E stays small.  Prob mode; three far sequences against a
    call on those sequences alone with the same chunk length: both calls are the same fp32 algorithm on the same plan
    per sequence, so the class sums and dE rows are held to each other bit for bit."""
    k, b, L, q, C = 1, 2048, 65600, 2, 16
    assert b * L * C > 2 ** 31 > b * L * q
    table = [3, 15]
    rng = np.random.default_rng(12)
    A, pi = ps.build_model(rng, "dense", q)
    A, pi = dev(A[None]), dev(pi[None])
    g = torch.Generator(device=DEV).manual_seed(9)
    E = torch.rand((k, b, L, q), generator=g, device=DEV) * 0.9 + 0.05
    G = torch.zeros((k, b, L, C), device=DEV)
    G[..., 3] = torch.randn((k, b, L), generator=g, device=DEV)
    G[..., 15] = torch.randn((k, b, L), generator=g, device=DEV)
    rows = [0, 1027, b - 1]
    with engine.option(engine.OPT_CHUNK, 256):
        P, _, ll = engine.class_posterior(A, pi, E, table, C)
        dA, dpi, dE = engine.class_posterior_grad(A, pi, E, table, C, G, mode=engine.POST_PROB)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(dA).all()) and bool(torch.isfinite(dpi).all())
        gotP, gotE, gotll = P[0, rows].cpu(), dE[0, rows].cpu(), ll[0, rows].cpu()
        tail = P[0, -1, -4:].cpu()
        del P, dA, dpi, dE
        engine.release_workspaces()
        torch.cuda.empty_cache()
        Es, Gsub = E[:, rows].contiguous(), G[:, rows].contiguous()
        del E, G
        torch.cuda.empty_cache()
        P3, _, ll3 = engine.class_posterior(A, pi, Es, table, C)
        dE3 = engine.class_posterior_grad(A, pi, Es, table, C, Gsub, mode=engine.POST_PROB)[2]
        torch.cuda.synchronize()
    assert torch.equal(gotP, P3[0].cpu()) and torch.equal(gotll, ll3[0].cpu())
    assert torch.equal(gotE, dE3[0].cpu())
    assert bool(torch.isfinite(gotE).all()) and float(gotE.abs().max()) > 0
    assert bool((tail[:, [3, 15]].sum(-1) - 1).abs().max() < 1e-5) and bool((tail[:, :3] == 0).all())
    engine.release_workspaces()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("log", cc.MODES)
def test_autograd_node_against_fp64_cpu_autograd(log):
    spec = [s for s in cc.state_sweep() if s.models == ("gene",) and s.table == "gene" and s.log == log][0]
    c = cc.build(spec)
    table, C = cc.table_of(spec)
    A, pi, E, G = c["A"], c["pi"], c["E"], c["G"]
    leaves = [dev(x).requires_grad_(True) for x in (A, pi, E)]
    out = autograd.class_posterior(*leaves, list(table), C, mode=mode_of(log), fused=True)
    assert out.shape == (1, spec.b, spec.L, C) and type(out.grad_fn).__name__.startswith("ClassPosteriorSmall")
    (out * dev(G)).sum().backward()
    torch.cuda.synchronize()
    full = cw.oracle(A[0], pi[0], E[0], G[0], table, C, log)
    for name, t, w in zip(("dA", "dpi", "dE"), leaves, full[:3]):
        got = t.grad[0].cpu().numpy()
        err = np.abs(got - w).max()
        print("CPSWEEP autograd %s %s err %.3e max|want| %.3e" % ("log" if log else "prob", name, err, np.abs(w).max()))
        assert err <= cc.TENSOR_REL * np.abs(w).max() + cc.TENSOR_ABS, (name, err)
    fwd = out[0].detach().cpu().numpy().astype(np.float64)
    n = dm.largest_class(table, C)
    assert np.abs((np.exp(fwd) if log else fwd) - full[3]).max() <= n * dm.STATE_TOL
    # the composed route computes the same function
    plain = [dev(x).requires_grad_(True) for x in (A, pi, E)]
    out2 = autograd.class_posterior(*plain, list(table), C, mode=mode_of(log), fused=False)
    assert not type(out2.grad_fn).__name__.startswith("ClassPosteriorSmall")
    fwd2 = out2[0].detach().cpu().numpy().astype(np.float64)
    assert np.abs((np.exp(fwd2) if log else fwd2) - full[3]).max() <= n * dm.STATE_TOL


def test_gene_layer_trains_through_the_class_posteriors(monkeypatch):
    """loss.backward() through class_posterior_log_probs(x, classes, training=True) of the 15-state layer: one
    hmm_class_posterior and one hmm_class_posterior_grad where the predicate says 1 (a table of measurements: played
    here), no engine.posterior.  Parameter gradients against fp64 CPU autograd through the same cell's producers, within
    the tolerance of tests/test_layer_gpu.py::test_training_through_state_posteriors (2e-3 of the largest entry)."""
    from oracle import torch64
    b, L, q = 3, 250, 15
    table, C = dm.gene_classes(q), 6
    cell, x, _, _, _ = gene_setup(b, L, seed=8)
    host = gene_setup(b, L, seed=8, device="cpu")[0]
    labels = torch.nn.functional.one_hot(torch.randint(0, C, (b, L), generator=torch.Generator().manual_seed(3)), C).float()
    calls = []
    for name in ("class_posterior", "class_posterior_grad", "posterior", "posterior_grad"):
        def spy(*a, _real=getattr(engine, name), _name=name, **kw):
            calls.append(_name)
            return _real(*a, **kw)
        monkeypatch.setattr(engine, name, spy)
    monkeypatch.setattr(engine.lib(), "hmm_class_posterior_grad_pays", lambda *dims: 1)
    layer = MsaHmmLayer(cell, use_prior=False)
    layer.build(x.shape)
    logp = layer.class_posterior_log_probs(x, table, training=True)
    assert calls == ["class_posterior"] and logp.shape == (1, b, L, C) and logp.requires_grad
    loss = -(labels.to(DEV) * logp[0]).mean()
    loss.backward()
    assert calls == ["class_posterior", "class_posterior_grad"], calls
    host.recurrent_init()
    E = host.emission_probs(x.cpu(), end_hints=None, training=True).to(torch.float64)
    gam, _ = torch64.posterior(host.A.to(torch.float64)[0], host.init_dist.to(torch.float64).reshape(q), E[0], host.epsilon)
    P = gam @ torch.tensor(cw.one_hot(table, C))
    ref_loss = -(labels.double() * torch.log(P)).mean()
    assert abs(float(loss) - float(ref_loss)) <= 1e-4 * abs(float(ref_loss)) + 1e-4
    ref_loss.backward()
    checked = 0
    for (name, p), (_, r) in zip(cell.named_parameters(), host.named_parameters()):
        if r.grad is None:
            continue
        want, got = r.grad, p.grad.cpu()
        scale, err = float(want.abs().max()), float((got - want).abs().max())
        print("CPSWEEP layer %s err %.3e max|want| %.3e" % (name, err, scale))
        assert bool(torch.isfinite(got).all()) and err <= 2e-3 * scale + 1e-7, (name, err, scale)
        checked += 1
    assert checked >= 2
    # without gradients the layer takes the fused forward where hmm_class_posterior_pays says 1, else composes
    del calls[:]
    with torch.no_grad():
        monkeypatch.setattr(engine.lib(), "hmm_class_posterior_pays", lambda *dims: 1)
        fused = layer.class_posterior_log_probs(x, table)
        monkeypatch.setattr(engine.lib(), "hmm_class_posterior_pays", lambda *dims: 0)
        composed = layer.class_posterior_log_probs(x, table)
    assert calls == ["class_posterior", "posterior"], calls
    assert float((fused.exp() - composed.exp()).abs().max()) <= 1e-6
