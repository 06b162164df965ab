"""hmm_class_posterior_walk / hmm_class_posterior_grad_walk (engine.class_posterior_walk, engine.
class_posterior_grad_walk; 65..256 states) on the device.

Forward: the bit-identities with hmm_posterior_decode_wide and hmm_posterior_walk on the same table, out_log against
out_prob, out_prob against fp64 sums of the walk's own gamma and against the fp64 oracle.  Backward: prob mode bit for
bit hmm_posterior_grad_walk with the gradient expanded to the states, log mode the same with G' = Gc / P computed here
in numpy fp32 from the engine's out_prob; every case of tests/class_posterior_walk_cases.py against the fp64 oracle
under the project's four norms (that module's docstring; nothing in a limit comes from engine output) with exact zeros
in dA wherever A == 0.  And the properties the header promises: refusal next to a served model, an empty class,
determinism on a workspace of NaN bytes, k = 2 against two k = 1 calls, graph capture of both calls with the host table
overwritten after capture, offsets beyond 2^31 elements, the autograd node and the five-copy layer."""
import ctypes

import numpy as np
import pytest
import torch

from hmm_layer_amd import autograd, engine

import class_posterior_walk_cases as cc
import posterior_decode_mid_cases as dm
import postgrad_mid_cases as pm
from test_loglik_grad_large_gpu import CODONS, five_copy

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FWD_SPECS = [s for s in cc.gene_sweep() + cc.state_sweep() + cc.length_sweep() + cc.eps_cases() + cc.table_cases()
             if not s.log]


def dev(x):
    return torch.as_tensor(np.asarray(x), dtype=torch.float32, device=DEV)


def mode_of(log):
    return engine.POST_LOG if log else engine.POST_PROB


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def ctable(table):
    return (ctypes.c_int * len(table))(*table)


def forward(c, spec, prob=True, log=True):
    """-> numpy (prob, log, loglik) of engine.class_posterior_walk on the case's inputs."""
    table, C = cc.table_of(spec)
    out = engine.class_posterior_walk(dev(c["A"]), dev(c["pi"]), dev(c["E"]), list(table), C, eps=spec.eps, prob=prob,
                                      log=log)
    torch.cuda.synchronize()
    return [None if t is None else t.cpu().numpy() for t in out]


def backward(A, pi, E, G, P, table, C, log, eps=cc.EPS, **kw):
    """numpy in -> numpy (dA, dpi, dE) of engine.class_posterior_grad_walk."""
    out = engine.class_posterior_grad_walk(dev(A), dev(pi), dev(E), list(table), C, dev(G),
                                           class_prob=None if P is None else dev(P), mode=mode_of(log), eps=eps, **kw)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def state_backward(A, pi, E, G, eps=cc.EPS, **kw):
    out = engine.posterior_grad_walk(dev(A), dev(pi), dev(E), dev(G), mode=engine.POST_PROB, eps=eps, **kw)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def quotient(G, P):
    """G' of the header in numpy fp32: the IEEE quotient, 0 where the class posterior is 0."""
    G, P = np.asarray(G, np.float32), np.asarray(P, np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(P > 0, G / P, np.float32(0)).astype(np.float32)


def same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def held(got, ref_m, A, tag):
    """One model under every norm the case is held to; prints each figure, then asserts."""
    err, limit, off = cc.check(got, ref_m, A)
    for n in limit:
        print("CPWSWEEP %s %s err %.3e limit %.3e e32 %.3e" % (tag, n, err[n], limit[n], ref_m["e32"][n]))
    print("CPWSWEEP %s off-support non-zeros %d" % (tag, off))
    assert all(np.isfinite(x).all() for x in got), tag
    bad = [(n, err[n], limit[n]) for n in limit if not err[n] <= limit[n]]
    assert not bad and off == 0, (tag, bad, off)


def decode_wide(c, spec):
    """hmm_posterior_decode_wide itself (engine.posterior_decode may compose) -> numpy (label, conf, loglik)."""
    table, C = cc.table_of(spec)
    A, pi, E = dev(c["A"]), dev(c["pi"]), dev(c["E"])
    k, b, L, q = E.shape
    lib = engine.lib()
    need = lib.hmm_posterior_decode_wide_workspace_bytes(k, b, L, q)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    label = torch.empty((k, b, L), dtype=torch.uint8, device=DEV)
    conf = torch.empty((k, b, L), dtype=torch.float32, device=DEV)
    ll = torch.empty((k, b), dtype=torch.float64, device=DEV)
    rc = lib.hmm_posterior_decode_wide(A.data_ptr(), pi.data_ptr(), E.data_ptr(), k, b, L, q, spec.eps, ctable(table), C,
                                       label.data_ptr(), conf.data_ptr(), ll.data_ptr(), ws.data_ptr(), need, stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return label.cpu().numpy(), conf.cpu().numpy(), ll.cpu().numpy()


@pytest.mark.parametrize("spec", FWD_SPECS, ids=cc.spec_id)
def test_forward(spec):
    c, refs = cc.build(spec), cc.reference(spec)
    table, C = cc.table_of(spec)
    n = dm.largest_class(table, C)
    P, Lg, ll = forward(c, spec)
    # the bits hmm_posterior_decode_wide compares, and hmm_posterior_walk's log-likelihood
    label, conf, ll_dec = decode_wide(c, spec)
    assert np.array_equal(np.take_along_axis(P, label[..., None].astype(np.int64), -1)[..., 0], conf)
    assert np.array_equal(P.argmax(-1), label)                                  # (numpy: the first maximal index)
    gamma, ll_walk = engine.posterior_walk(dev(c["A"]), dev(c["pi"]), dev(c["E"]), mode=engine.POST_PROB, eps=spec.eps)
    assert np.array_equal(ll, ll_walk.cpu().numpy()) and np.array_equal(ll, ll_dec)
    # one output or both: the same bits
    assert np.array_equal(forward(c, spec, log=False)[0], P)
    assert np.array_equal(forward(c, spec, prob=False)[1], Lg, equal_nan=True)
    # out_log against out_prob: 2 ulp of fp32 around log in fp64, -inf exactly at 0
    zero = P == 0
    assert np.all(np.isneginf(Lg[zero])) and np.all(np.isfinite(Lg[~zero]))
    want = np.log(P[~zero].astype(np.float64))
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    worst = float((np.abs(Lg[~zero] - want) / ulp).max()) if want.size else 0.0
    print("CPWSWEEP %s log: %.2f ulp" % (cc.spec_id(spec), worst))
    assert worst <= 2.0
    used = np.bincount(np.asarray(table), minlength=C) > 0
    assert np.all(zero[..., ~used])                                             # an empty class: exactly 0 and -inf
    # out_prob against fp64 sums of the walk's own gamma
    sums = gamma.cpu().numpy().astype(np.float64) @ cc.one_hot(table, C)
    err = float(np.abs(P - sums).max())
    print("CPWSWEEP %s own gamma: err %.3e tol %.3e" % (cc.spec_id(spec), err, dm.tol(n)))
    assert err <= dm.tol(n)
    # ... and against the oracle; rows sum to 1
    for m, ref in enumerate(refs):
        err = float(np.abs(P[m] - ref["P"]).max())
        one = float(np.abs(P[m].astype(np.float64).sum(-1) - 1).max())
        print("CPWSWEEP %s m=%d oracle: err %.3e rows %.3e bound %.3e" % (cc.spec_id(spec), m, err, one, n * dm.STATE_TOL))
        assert err <= n * dm.STATE_TOL and one <= n * dm.STATE_TOL


@pytest.mark.parametrize("spec", cc.all_specs(), ids=cc.spec_id)
def test_backward(spec):
    c, refs = cc.build(spec), cc.reference(spec)
    table, C = cc.table_of(spec)
    A, pi, E, G = c["A"], c["pi"], c["E"], c["G"]
    P = forward(c, spec, log=False)[0]
    got = backward(A, pi, E, G, P if spec.log else None, table, C, spec.log, spec.eps)
    # the state-level call with the gradient expanded to the states (log mode: G' first), bit for bit
    Gs = cc.expand(quotient(G, P) if spec.log else G, table)
    assert same(got, state_backward(A, pi, E, Gs, spec.eps))
    for m in range(len(spec.models)):
        held([x[m] for x in got], refs[m], A[m], "%s m=%d" % (cc.spec_id(spec), m))
        assert np.all(got[2][m][E[m] <= spec.eps] == 0.0)
        assert np.all(got[1][m][pi[m] <= spec.eps] == 0.0)
    if spec.L == 1:
        assert np.all(got[0] == 0.0)


@pytest.mark.parametrize("spec", cc.refused_cases(), ids=cc.spec_id)
def test_refused_model_next_to_a_served_one(spec):
    c, refs = cc.build(spec), cc.reference(spec)
    table, C = cc.table_of(spec)
    assert spec.models[0] == cc.REFUSED and refs[0] is None
    A, pi, E, G = c["A"], c["pi"], c["E"], c["G"]
    dims = E.shape
    P = forward(c, spec, log=False)[0]                                          # the forward serves every model (dense step)
    assert np.isfinite(P).all()
    got = backward(A, pi, E, G, P, table, C, spec.log, check=False)
    assert engine.class_posterior_grad_walk_refused(dims) == 1
    alone = backward(A[1:], pi[1:], E[1:], G[1:], P[1:], table, C, spec.log)
    assert engine.class_posterior_grad_walk_refused((1,) + dims[1:]) == 0
    for x, y in zip(got, alone):
        assert np.isnan(x[0]).all()                                            # every output element of the refused model
        assert np.array_equal(x[1:], y)                                        # the served one: its own k = 1 call
    held([x[1] for x in got], refs[1], A[1], cc.spec_id(spec) + " m=1")
    with pytest.raises(engine.EngineError, match="refused"):
        backward(A, pi, E, G, P, table, C, spec.log, check=True)


@pytest.mark.parametrize("log", cc.MODES)
def test_an_empty_class_passes_nothing(log):
    spec = cc.table_cases()[int(log)]                                           # gene + deg1, 71 states, dense Gc
    assert (spec.table, spec.G, spec.log) == ("empty", "dense", log)
    c = cc.build(spec)
    table, C = cc.table_of(spec)
    P, Lg, _ = forward(c, spec)
    assert np.all(P[..., cc.EMPTY_CLASS] == 0.0) and np.all(np.isneginf(Lg[..., cc.EMPTY_CLASS]))
    G = np.array(c["G"])
    assert np.all(G[..., cc.EMPTY_CLASS] != 0.0)
    got = backward(c["A"], c["pi"], c["E"], G, P, table, C, log)
    assert all(np.isfinite(x).all() for x in got)
    G[..., cc.EMPTY_CLASS] = 0.0                                                # the same call without its gradient
    assert same(got, backward(c["A"], c["pi"], c["E"], G, P, table, C, log))
    G[...] = 0.0
    G[..., cc.EMPTY_CLASS] = 7.0                                                # ... and that gradient alone
    assert all(np.all(x == 0.0) for x in backward(c["A"], c["pi"], c["E"], G, P, table, C, log))


def raw_forward(A, pi, E, ctab, C, P, Lg, ll, ws, eps=cc.EPS):
    k, b, L, q = E.shape
    rc = engine.lib().hmm_class_posterior_walk(A.data_ptr(), pi.data_ptr(), E.data_ptr(), k, b, L, q, eps, ctab, C,
                                               P.data_ptr(), Lg.data_ptr(), ll.data_ptr(), ws.data_ptr(), ws.numel(),
                                               stream())
    assert rc == 0, rc


def raw_backward(A, pi, E, mode, ctab, C, P, G, outs, ws, eps=cc.EPS):
    k, b, L, q = E.shape
    rc = engine.lib().hmm_class_posterior_grad_walk(A.data_ptr(), pi.data_ptr(), E.data_ptr(), k, b, L, q, eps, mode,
                                                    ctab, C, P.data_ptr(), G.data_ptr(), *(t.data_ptr() for t in outs),
                                                    ws.data_ptr(), ws.numel(), stream())
    assert rc == 0, rc


@pytest.mark.parametrize("log", cc.MODES)
def test_repeated_calls_on_workspaces_of_nan_bytes(log):
    spec = cc.batch_sweep()[4 + int(log)]                                      # gene + deg2, 127 states, b = 65
    assert (spec.b, spec.log, len(spec.models)) == (65, log, 2)
    c = cc.build(spec)
    table, C = cc.table_of(spec)
    ctab = ctable(table)
    A, pi, E, G = dev(c["A"]), dev(c["pi"]), dev(c["E"]), dev(c["G"])
    k, b, L, q = E.shape
    lib = engine.lib()
    wf = torch.zeros(lib.hmm_class_posterior_walk_workspace_bytes(k, b, L, q), dtype=torch.uint8, device=DEV)
    need = lib.hmm_class_posterior_grad_walk_workspace_bytes(k, b, L, q, C)
    wb = torch.zeros(need, dtype=torch.uint8, device=DEV)
    fwd = [torch.zeros((k, b, L, C), device=DEV), torch.zeros((k, b, L, C), device=DEV),
           torch.zeros((k, b), dtype=torch.float64, device=DEV)]
    outs = [torch.zeros((k, q, q), device=DEV), torch.zeros((k, q), device=DEV), torch.zeros_like(E)]
    raw_forward(A, pi, E, ctab, C, *fwd, wf)
    raw_backward(A, pi, E, mode_of(log), ctab, C, fwd[0], G, outs, wb)
    torch.cuda.synchronize()
    first = [t.clone() for t in fwd + outs]
    assert lib.hmm_posterior_grad_walk_refused(k, b, L, q, wb.data_ptr(), need) == 0       # the state call's reader
    P = fwd[0].clone()
    for ws in (wf, wb):
        ws.fill_(0xFF)                                                         # every float a NaN
    for t in fwd + outs:
        t.fill_(float("nan"))
    raw_forward(A, pi, E, ctab, C, *fwd, wf)
    raw_backward(A, pi, E, mode_of(log), ctab, C, P, G, outs, wb)
    torch.cuda.synchronize()
    for x, y in zip(first, fwd + outs):
        assert torch.equal(x, y) and bool(torch.isfinite(y).all())
    assert lib.hmm_posterior_grad_walk_refused(k, b, L, q, wb.data_ptr(), need) == 0


@pytest.mark.parametrize("log", cc.MODES)
def test_two_models_are_two_calls(log):
    spec = cc.length_sweep()[16 + int(log)]                                    # gene + deg1, 71 states, L = 17
    assert (spec.q, spec.L, spec.log, len(spec.models)) == (71, 17, log, 2)
    c = cc.build(spec)
    table, C = cc.table_of(spec)
    fwd = forward(c, spec)
    both = backward(c["A"], c["pi"], c["E"], c["G"], fwd[0], table, C, log)
    for m in range(2):
        one = {n: c[n][m:m + 1] for n in c}
        fwd1 = forward(one, spec)
        assert same([x[m:m + 1] for x in fwd], fwd1), m
        alone = backward(one["A"], one["pi"], one["E"], one["G"], fwd1[0], table, C, log)
        assert same([x[m:m + 1] for x in both], alone), m


def test_graph_capture_and_replay_keeps_the_table():
    spec = cc.gene_sweep()[7]                                                  # the nine-copy model, holes, log mode
    assert (spec.q, spec.emis, spec.log) == (127, "holes", True)
    c = cc.build(spec)
    table, C = cc.table_of(spec)
    ctab = ctable(table)
    A, pi = dev(c["A"]), dev(c["pi"])
    E, G = dev(c["E"][:, :, :50]), dev(c["G"][:, :, :50])
    E2, G2 = dev(np.ascontiguousarray(c["E"][:, :, 50:100])), dev(np.ascontiguousarray(c["G"][:, :, 50:100]))
    k, b, L, q = E.shape
    lib = engine.lib()
    wf = torch.empty(lib.hmm_class_posterior_walk_workspace_bytes(k, b, L, q), dtype=torch.uint8, device=DEV)
    wb = torch.empty(lib.hmm_class_posterior_grad_walk_workspace_bytes(k, b, L, q, C), dtype=torch.uint8, device=DEV)
    fwd = [torch.zeros((k, b, L, C), device=DEV), torch.zeros((k, b, L, C), device=DEV),
           torch.zeros((k, b), dtype=torch.float64, device=DEV)]
    outs = [torch.zeros((k, q, q), device=DEV), torch.zeros((k, q), device=DEV), torch.zeros_like(E)]
    g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.stream(s):
        raw_forward(A, pi, E, ctab, C, *fwd, wf)                               # (loads the kernels before the capture)
        raw_backward(A, pi, E, engine.POST_LOG, ctab, C, fwd[0], G, outs, wb)
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):                                    # one stream, no host synchronisation
            raw_forward(A, pi, E, ctab, C, *fwd, wf)
            raw_backward(A, pi, E, engine.POST_LOG, ctab, C, fwd[0], G, outs, wb)
        for i in range(q):                                                     # the host table: read at capture, by value
            ctab[i] = 0
        E.copy_(E2)                                                            # capture does not run the kernels
        G.copy_(G2)
        for t in fwd + outs:
            t.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        wantf = engine.class_posterior_walk(A, pi, E2, list(table), C, log=True)
        wantb = engine.class_posterior_grad_walk(A, pi, E2, list(table), C, G2, class_prob=wantf[0])
        torch.cuda.synchronize()
    for x, y in zip(fwd + outs, list(wantf) + list(wantb)):
        assert torch.equal(x, y) and bool(torch.isfinite(y).all())


def test_offsets_beyond_2_to_31():
    """k*b*L*q > 2^31 elements: many short sequences, the shape of tests/test_posterior_grad_walk_gpu.py; three sampled
    sequences, the last included: the class posteriors against the oracle's, dE against the oracle under the tensor norm
    scaled by the sampled sequences' own maximum."""
    k, b, L, q = 1, 8192, 3700, 71
    assert k * b * L * q > 2 ** 31
    A, pi = five_copy()
    table, C = dm.gene_classes(q), 6
    g = torch.Generator(device=DEV).manual_seed(9)
    E = torch.rand((k, b, L, q), generator=g, device=DEV) * 0.9 + 0.05
    lab = torch.randint(0, C, (k, b, L), generator=g, device=DEV)
    G = -torch.nn.functional.one_hot(lab, C).float()
    del lab
    rows = [0, 4099, b - 1]
    full = cc.oracle(A, pi, E[0, rows].cpu().numpy(), G[0, rows].cpu().numpy(), table, C, True)
    P, _, _ = engine.class_posterior_walk(dev(A[None]), dev(pi[None]), E, table, C)
    engine.release_workspaces()                                                # (the parking region)
    dA, dpi, dE = engine.class_posterior_grad_walk(dev(A[None]), dev(pi[None]), E, table, C, G, class_prob=P)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(P).all()) and bool(torch.isfinite(dA).all()) and bool(torch.isfinite(dpi).all())
    assert bool(torch.isfinite(dE[0, -1]).all()) and bool(torch.isfinite(dE[0, :, -1]).all())
    assert bool((dA[0][dev(A) == 0] == 0).all())
    gotP, got = P[0, rows].cpu().numpy(), dE[0, rows].cpu().numpy()
    del dA, dpi, dE, E, G, P
    engine.release_workspaces()
    torch.cuda.empty_cache()
    n = dm.largest_class(table, C)
    assert np.abs(gotP - full[3]).max() <= n * dm.STATE_TOL
    want = full[2]
    err = np.abs(got - want).max((1, 2))
    print("CPWSWEEP offsets err", err, "scale", np.abs(want).max((1, 2)))
    assert np.all(err <= pm.TENSOR_REL * np.abs(want).max((1, 2)) + pm.TENSOR_ABS), err


@pytest.mark.parametrize("log", cc.MODES)
def test_autograd_node_against_fp64_cpu_autograd(log):
    spec = cc.length_sweep()[16 + int(log)]._replace(models=("gene",))          # 71 states, L = 17, dense Gc
    c = cc.build(spec)
    table, C = cc.table_of(spec)
    A, pi, E, G = c["A"], c["pi"], c["E"], c["G"]
    assert A.shape == (1, 71, 71) and G.shape[-1] == C == 6
    leaves = [dev(x).requires_grad_(True) for x in (A, pi, E)]
    out = autograd.class_posterior(*leaves, list(table), C, mode=mode_of(log), support_only="always")
    assert out.shape == (1, spec.b, spec.L, C) and out.grad_fn is not None
    assert type(out.grad_fn).__name__.startswith("ClassPosterior")
    (out * dev(G)).sum().backward()
    torch.cuda.synchronize()
    full = cc.oracle(A[0], pi[0], E[0], G[0], table, C, log)
    present = A[0] > 0
    got = [t.grad[0].cpu().numpy() for t in leaves]
    want = cc.on_support(full[:3], A[0])
    assert np.all(got[0][~present] == 0.0) and np.abs(full[0][~present]).max() > 0          # dense autograd fills them
    for name, g, w in zip(("dA", "dpi", "dE"), got, want):
        err = np.abs(g - w).max()
        print("CPWSWEEP autograd %s %s err %.3e max|want| %.3e" % ("log" if log else "prob", name, err, np.abs(w).max()))
        assert err <= pm.TENSOR_REL * np.abs(w).max() + pm.TENSOR_ABS, (name, err)
    fwd = out[0].detach().cpu().numpy().astype(np.float64)
    n = dm.largest_class(table, C)
    assert np.abs((np.exp(fwd) if log else fwd) - full[3]).max() <= n * dm.STATE_TOL
    # the composed route (the default) computes the same function: its dA has the absent edges' derivatives
    plain = [dev(x).requires_grad_(True) for x in (A, pi, E)]
    out2 = autograd.class_posterior(*plain, list(table), C, mode=mode_of(log))
    (out2 * dev(G)).sum().backward()
    assert float(plain[0].grad[0][torch.as_tensor(~present, device=DEV)].abs().max()) > 0
    fwd2 = out2[0].detach().cpu().numpy().astype(np.float64)
    assert np.abs((np.exp(fwd2) if log else fwd2) - full[3]).max() <= n * dm.STATE_TOL


def test_five_copy_layer_trains_through_the_class_posteriors(monkeypatch):
    """loss.backward() through class_posterior_log_probs(x, classes, training=True) of the 71-state layer with
    support_grad=True: one hmm_class_posterior_walk and one hmm_class_posterior_grad_walk where the predicate says 1 (a
    table of measurements: played here).  The gradients of the transition and emission kernels against autograd through
    the same cell's torch ops on the CPU with the HMM recursion, the class sums and the logs in fp64, within the
    tolerance of test_five_copy_layer_with_support_grad (5e-4 of the largest entry)."""
    from hmm_layer_amd.MsaHmmCell import HmmCell
    from hmm_layer_amd.MsaHMMLayer import MsaHmmLayer
    from hmm_layer_amd.gene_pred_hmm_emitter import GenePredHMMEmitter
    from hmm_layer_amd.gene_pred_hmm_transitioner import GenePredMultiHMMTransitioner
    from oracle import torch64
    b, L, q, C = 2, 160, 71, 6
    table = dm.gene_classes(q)
    g = torch.Generator().manual_seed(13)
    cls = torch.softmax(2 * torch.randn((1, b, L, 15), generator=g), -1)
    nuc = torch.nn.functional.one_hot(torch.randint(0, 4, (1, b, L), generator=g), 5).float()
    x = torch.cat([cls, nuc], -1)
    labels = torch.nn.functional.one_hot(torch.randint(0, C, (b, L), generator=g), C).float()
    calls = []
    for name in ("class_posterior_walk", "class_posterior_grad_walk", "posterior_walk", "posterior_grad_walk", "posterior"):
        def spy(*a, _real=getattr(engine, name), _name=name, **kw):
            calls.append(_name)
            return _real(*a, **kw)
        monkeypatch.setattr(engine, name, spy)
    monkeypatch.setattr(engine.lib(), "hmm_class_posterior_walk_pays", lambda *dims: 1)

    def make():
        torch.manual_seed(5)
        np.random.seed(5)
        em = GenePredHMMEmitter(**CODONS, num_copies=5)
        em.build((1, b, L, 15))
        tr = GenePredMultiHMMTransitioner(k=5, initial_exon_len=200, initial_intron_len=4500, initial_ir_len=10000,
                                          support_grad=True)
        return HmmCell([q], 15, em, tr)

    host, cell = make(), make().to(DEV)
    assert all(torch.equal(p.detach().cpu(), r.detach()) for p, r in zip(cell.parameters(), host.parameters()))
    layer = MsaHmmLayer(cell, use_prior=False)
    layer.build(x.shape)
    logp = layer.class_posterior_log_probs(x.to(DEV), table, training=True)
    assert calls == ["class_posterior_walk"] and logp.shape == (1, b, L, C)
    loss = -(labels.to(DEV) * logp[0]).mean()
    loss.backward()
    assert calls == ["class_posterior_walk", "class_posterior_grad_walk"], calls
    # the reference: the cell's own torch ops on the CPU, then fp64
    host.recurrent_init()
    E = host.emission_probs(x, end_hints=None, training=True).to(torch.float64)
    A = host.A.to(torch.float64)[0]
    pi = host.init_dist.to(torch.float64).reshape(q)
    gam, _ = torch64.posterior(A, pi, E[0], host.epsilon)
    P = gam @ torch.tensor(cc.one_hot(table, C))
    (-(labels.double() * torch.log(P)).mean()).backward()
    n = 0
    for (name, p), (_, r) in zip(cell.named_parameters(), host.named_parameters()):
        if r.grad is None:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, name
            continue
        want, got = r.grad, p.grad.cpu()
        err = float((got - want).abs().max())
        print("CPWSWEEP layer %s err %.3e max|want| %.3e" % (name, err, float(want.abs().max())))
        assert bool(torch.isfinite(got).all()) and float(want.abs().max()) > 0
        assert err <= 5e-4 * float(want.abs().max()) + 1e-7, name
        n += 1
    assert n >= 2                                                               # the transition and the emission kernels
    # without gradients the layer takes the fused forward for this model, or composes: the same numbers
    del calls[:]
    with torch.no_grad():
        fused = layer.class_posterior_log_probs(x.to(DEV), table)
        monkeypatch.setattr(engine.lib(), "hmm_posterior_walk_pays", lambda *dims: 0)
        composed = layer.class_posterior_log_probs(x.to(DEV), table)
    assert calls == ["class_posterior_walk", "posterior"], calls
    bound = 2 * dm.largest_class(table, C) * dm.STATE_TOL                       # each within n STATE_TOL of the truth
    assert float((fused.exp() - composed.exp()).abs().max()) <= bound
    assert float((fused.exp() - logp.detach().exp()).abs().max()) <= bound
