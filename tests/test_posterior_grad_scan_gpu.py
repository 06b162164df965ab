"""hmm_posterior_grad_scan: the posterior gradients per chunk of the scan plan for every model of 17..64 states
(csrc/hmm_postgrad_scan.inc; rows of 32 lanes up to 32 states, of 64 above).  Needs an MI355X.

Inputs: tests/postgrad_scan_cases.py; tests/test_posterior_grad_scan_cpu.py shows from fp64 alone that they can carry
the assertions made here.  Oracle: oracle/torch64.py by fp64 autograd, under the four norms of
tests/postgrad_mid_cases.py — per tensor 3e-4 * max|want| + 1e-6; dE per state column, dE per sequence and dA per row
over present edges max(3e-4, 4 e32), e32 = the error of fp32 autograd through the same recursion.  Against the
whole-sequence sweeps of hmm_posterior_grad (OPT_PGCHUNK = 0): 1e-4 * max + 1e-7 per tensor, the figure of the
29-state test (tests/test_postgrad_chunked_gpu.py).  Each comparison prints its figures (pytest -s) before it asserts.

Shapes: a full row (32, 64 states) and one past it (33, 49), both row widths, all three instantiations of the redo
(q <= 32, <= 48, <= 64), ragged last chunks (L / chunk = 333 / 16, 97 / 16, 2100 / 64, 700 / the plan's own), odd
numbers of chains for the two-rows-per-wave width (3 * 21, 5 * 7), several models; the compiled 29-state topology (the
sparse reduce and its pad-lane marks) once.

Worst error / limit measured on an MI355X over the parity cases, per norm, with the case's e32:
    tensor   0.006  (1.7e-6 of 3e-4,    gene-q43-b2-L700-T0-prob);   e32 1.6e-6
    dE/col   0.001  (2.8e-7 of 3e-4,    dense-q24-b3-L333-T16-prob); e32 3.4e-7
    dE/seq   0.010  (3.0e-6 of 3e-4,    gene-q43-b3-L333-T16-prob);  e32 2.3e-6
    dA/row   0.153  (5.4e-4 of 3.53e-3, gene-q43-b3-L333-T16-prob);  e32 8.8e-4
Against the whole-sequence sweeps at most 6.4e-6 of a tensor's maximum (dA, gene-q43-b1-L2100-T64-log).
"""
import ctypes

import numpy as np
import pytest
import torch

from hmm_layer_amd import engine

import postgrad_scan_cases as sc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CODONS = dict(start_codons=[("ATG", 1.)], stop_codons=[("TAG", .34), ("TAA", .33), ("TGA", .33)],
              intron_begin_pattern=[("NGT", .99), ("NGC", .005), ("NAT", .005)],
              intron_end_pattern=[("AGN", .99), ("ACN", .01)])


def dev(x):
    return torch.as_tensor(np.array(x, dtype=np.float32, order="C"), device=DEV)    # (a copy: the cases are read-only)


def mode_of(log):
    return engine.POST_LOG if log else engine.POST_PROB


def run(fn, c, log):
    out = fn(dev(c["A"]), dev(c["pi"]), dev(c["E"]), dev(c["G"]), mode=mode_of(log))
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def scan(c, log):
    """-> (dA, dpi, dE) of hmm_posterior_grad_scan, and how many sequences the whole-sequence sweeps redid."""
    got = run(engine.posterior_grad_scan, c, log)
    return got, engine.posterior_grad_scan_serial_count(c["E"].shape)


def sweeps(c, log):
    """hmm_posterior_grad's whole-sequence sweeps."""
    with engine.option(engine.OPT_PGCHUNK, 0):
        got = run(engine.posterior_grad, c, log)
        assert engine.posterior_grad_serial_count(c["E"].shape) == c["E"].shape[0] * c["E"].shape[1]
    return got


def check_oracle(tag, got, c, refs):
    """Every model of the call under the four norms; refs: per model dict(want, limit, e32)."""
    failed = []
    for m, r in enumerate(refs):
        mine = [x[m] for x in got]
        assert all(np.isfinite(x).all() for x in mine), (tag, m)
        err, _ = sc.errors(mine, r["want"], c["A"][m])
        for norm, lim in sc.limits(r).items():
            print("PGSCAN %s m=%d %s err %.3e limit %.3e e32 %.3e ratio %.3f"
                  % (tag, m, norm, err[norm], lim, r["e32"].get(norm, 0.0), err[norm] / lim))
            if not err[norm] <= lim:
                failed.append((m, norm, err[norm], lim))
    assert not failed, (tag, failed)


def reference_of(c, log):
    """The oracle and the limits of inputs outside the case list, per model."""
    out = []
    for m in range(c["A"].shape[0]):
        want = sc.oracle(c["A"][m], c["pi"][m], c["E"][m], c["G"][m], log)
        twin = sc.oracle(c["A"][m], c["pi"][m], c["E"][m], c["G"][m], log, torch.float32)
        e32, _ = sc.errors(twin, want, c["A"][m])
        out.append(dict(want=want, e32=e32, limit={n: max(sc.FINE_FLOOR, sc.FINE_FACTOR * e32[n]) for n in sc.FINE_NORMS}))
    return out


def close_to_sweeps(tag, got, ser):
    for name, s_, c_ in zip(("dA", "dpi", "dE"), ser, got):
        d, top = np.abs(s_ - c_).max(), np.abs(s_).max()
        print("PGSCAN %s %s against the sweeps: %.3e of max %.3e" % (tag, name, d, top))
        assert d <= 1e-4 * top + 1e-7, (tag, name, d, top)


# ---- 1. parity ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sc.all_cases(), ids=sc.case_id)
def test_parity(case):
    c = sc.build(case)
    dims = c["E"].shape
    with engine.option(engine.OPT_CHUNK, case.chunk):
        assert 0 < engine.lib().hmm_posterior_grad_scan_chunk_len(*dims) < case.L      # more than one chunk
        got, n = scan(c, case.log)
    assert n == 0                                             # every sequence per chunk
    check_oracle(sc.case_id(case), got, c, [sc.reference(case)])
    close_to_sweeps(sc.case_id(case), got, sweeps(c, case.log))
    if not case.log:
        holes = c["E"][0] <= sc.EPS
        assert holes.any() and np.all(got[2][0][holes] == 0.0)


# ---- 2. several models in one call --------------------------------------------------------------------------------
@pytest.mark.parametrize("log", [False, True])
def test_several_models_in_one_call(log):
    """The gene model, a dense primitive model and a reducible one (block-diagonal A, 20 + 23 states: the whole-sequence
    sweeps redo its sequences, masked, in the same call)."""
    rng = np.random.default_rng(43)
    q, b, L = 43, 3, 300
    Ad, pid = sc.dense_model(rng, q)
    Ar = np.zeros((q, q), dtype=np.float32)
    Ar[:20, :20] = sc.dense_model(rng, 20)[0]
    Ar[20:, 20:] = sc.dense_model(rng, q - 20)[0]
    assert sc.primitive_power(Ar) is None and sc.primitive_power(Ad) is not None
    A = np.stack([np.array(sc.gene_model(3)[0]), Ad, Ar])
    pi = np.stack([pid, pid, pid])
    E = (rng.random((3, b, L, q)) * 0.9 + 0.05).astype(np.float32)
    if log:
        G = np.stack([-(g == g.max(-1, keepdims=True)).astype(np.float32)
                      for g in (sc.recursions64(A[m], pi[m], E[m])[0] for m in range(3))])
    else:
        G = rng.standard_normal(E.shape).astype(np.float32)
    c = dict(A=A, pi=pi, E=E, G=G)
    got, n = scan(c, log)
    assert n == b
    ser = sweeps(c, log)
    assert np.array_equal(got[2][2], ser[2][2]) and np.array_equal(got[0][2], ser[0][2])     # the redo IS the sweeps
    assert np.array_equal(got[1][2], ser[1][2])
    check_oracle("three models %s" % ("log" if log else "prob"), got, c, reference_of(c, log))


# ---- 3. routing per sequence --------------------------------------------------------------------------------------
@pytest.mark.parametrize("q", [43, 40])
def test_exposed_upstream_gradient_flags_every_sequence(q):
    """Log mode with a dense upstream gradient: every sequence goes to the whole-sequence sweeps, and every output is
    hmm_posterior_grad's under OPT_PGCHUNK = 0 bit for bit — at 43 states k_pg_*<48> behind rows of 64 lanes, at 40
    states the same on a dense model."""
    c = sc.flagged_case(q)
    with engine.option(engine.OPT_CHUNK, 16):
        got, n = scan(c, True)
    assert n == c["E"].shape[1]
    for s_, c_ in zip(sweeps(c, True), got):
        assert np.array_equal(s_, c_)


def test_floor_decided_sequence_is_redone():
    c = sc.floor_decided_case()
    got, n = scan(c, True)
    assert n == 1                                             # exactly that sequence
    ser = sweeps(c, True)
    assert np.array_equal(got[2][0, 1], ser[2][0, 1])
    for s in (0, 2):                                          # its neighbours are served per chunk
        assert not np.array_equal(got[2][0, s], ser[2][0, s])
        d, top = np.abs(got[2][0, s] - ser[2][0, s]).max(), np.abs(ser[2][0, s]).max()
        assert d <= 1e-4 * top + 1e-7, (s, d, top)
    check_oracle("floor-decided", got, c, reference_of(c, True))
    with engine.option(engine.OPT_PGCHUNK, 2):                # the hook: every sequence per chunk, no certificate
        _, n2 = scan(c, True)
    assert n2 == 0


# ---- 4. determinism and overwriting -------------------------------------------------------------------------------
def raw_call(c, log, fill=float("nan"), name="hmm_posterior_grad_scan"):
    """The C entry point on sentinel-filled outputs and a workspace of its own -> numpy dA, dpi, dE."""
    lib = engine.lib()
    k, b, L, q = c["E"].shape
    A, pi, E, G = dev(c["A"]), dev(c["pi"]), dev(c["E"]), dev(c["G"])
    ws = torch.empty(getattr(lib, name + "_workspace_bytes")(k, b, L, q), dtype=torch.uint8, device=DEV)
    dA = torch.full((k, q, q), fill, dtype=torch.float32, device=DEV)
    dpi = torch.full((k, q), fill, dtype=torch.float32, device=DEV)
    dE = torch.full((k, b, L, q), fill, dtype=torch.float32, device=DEV)
    rc = getattr(lib, name)(A.data_ptr(), pi.data_ptr(), E.data_ptr(), k, b, L, q, engine.EPS, mode_of(log), G.data_ptr(),
                            dA.data_ptr(), dpi.data_ptr(), dE.data_ptr(), ws.data_ptr(), ws.numel(),
                            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, rc
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in (dA, dpi, dE)]


@pytest.mark.parametrize("q,log", [(24, False), (57, True)])
def test_deterministic_and_everything_overwritten(q, log):
    case = [x for x in sc.all_cases() if (x.q, x.log, x.L) == (q, log, 333)][0]
    c = sc.build(case)
    with engine.option(engine.OPT_CHUNK, 48):
        one = raw_call(c, log)
        two = raw_call(c, log, fill=-7.0)
    for x, y in zip(one, two):
        assert np.isfinite(x).all()                           # no sentinel left: dA, dpi, all of dE
        assert np.array_equal(x, y)
    assert not np.any(two[2] == -7.0)


@pytest.mark.parametrize("q", [5, 16])
def test_sixteen_states_and_fewer_are_hmm_posterior_grad(q):
    rng = np.random.default_rng(q)
    A, pi = sc.dense_model(rng, q)
    E = (rng.random((1, 3, 400, q)) * 0.9 + 0.05).astype(np.float32)
    c = dict(A=A[None], pi=pi[None], E=E, G=rng.standard_normal(E.shape).astype(np.float32))
    for log in (False, True):
        mine, own = run(engine.posterior_grad_scan, c, log), run(engine.posterior_grad, c, log)
        for x, y in zip(mine, own):
            assert np.array_equal(x, y)
        assert engine.posterior_grad_scan_serial_count(E.shape) == engine.posterior_grad_serial_count(E.shape)


def test_workspace_reuse():
    """The engine keeps the workspace between calls: a small case, a larger one (the workspace grows), the small one
    again."""
    X = [x for x in sc.all_cases() if (x.q, x.log, x.L) == (33, False, 97)][0]
    Y = [x for x in sc.all_cases() if (x.q, x.log, x.L) == (64, False, 333)][0]
    engine.release_workspaces()
    with engine.option(engine.OPT_CHUNK, 16):
        first, _ = scan(sc.build(X), False)
        other, _ = scan(sc.build(Y), False)
        again, n = scan(sc.build(X), False)
    assert n == 0
    for a, b in zip(first, again):
        assert np.array_equal(a, b)
    check_oracle("reuse " + sc.case_id(Y), other, sc.build(Y), [sc.reference(Y)])
    check_oracle("reuse " + sc.case_id(X), again, sc.build(X), [sc.reference(X)])


# ---- 5. wrappers --------------------------------------------------------------------------------------------------
class _Answer:
    """Stands in for lib.hmm_posterior_grad_scan_pays on the Python side."""

    def __init__(self, value):
        self.value, self.asked = value, 0

    def __call__(self, *dims):
        self.asked += 1
        return self.value


def test_wrapper_routing(monkeypatch):
    """engine.posterior_grad takes hmm_posterior_grad_scan exactly where hmm_posterior_grad_scan_pays says so."""
    lib = engine.lib()
    case = [x for x in sc.all_cases() if (x.model, x.q, x.log, x.L) == ("gene", 43, True, 700)][0]
    c = sc.build(case)
    own = raw_call(c, True, name="hmm_posterior_grad")
    chunked = raw_call(c, True)
    assert not all(np.array_equal(x, y) for x, y in zip(own, chunked))      # the two paths differ in rounding
    for value, want in ((1, chunked), (0, own)):
        answer = _Answer(value)
        monkeypatch.setattr(lib, "hmm_posterior_grad_scan_pays", answer)
        got = run(engine.posterior_grad, c, True)
        assert answer.asked == 1
        for x, y in zip(got, want):
            assert np.array_equal(x, y)
        if value:
            assert engine.posterior_grad_scan_serial_count(c["E"].shape) == 0
    # 16 states and fewer never ask
    answer = _Answer(1)
    monkeypatch.setattr(lib, "hmm_posterior_grad_scan_pays", answer)
    rng = np.random.default_rng(3)
    A, pi = sc.dense_model(rng, 12)
    E = (rng.random((1, 2, 50, 12)) * 0.9 + 0.05).astype(np.float32)
    run(engine.posterior_grad, dict(A=A[None], pi=pi[None], E=E, G=np.ones_like(E)), True)
    assert answer.asked == 0


@pytest.mark.parametrize("no_loglik", [False, True])
def test_three_copy_layer_trains_the_same_either_way(monkeypatch, no_loglik):
    """A cross-entropy on MsaHmmLayer.state_posterior_log_probs(x, training=True) of the 43-state model: the parameter
    gradients with the posterior gradient taken per chunk equal those of the whole-sequence sweeps (tolerance of
    tests/test_loglik_grad_scan_gpu.py::test_three_copy_layer_trains_the_same_either_way); with no_loglik the autograd
    node composes POST_LOG_NO_LL around the same call."""
    from hmm_layer_amd.MsaHmmCell import HmmCell
    from hmm_layer_amd.MsaHMMLayer import MsaHmmLayer
    from hmm_layer_amd.gene_pred_hmm_emitter import GenePredHMMEmitter
    from hmm_layer_amd.gene_pred_hmm_transitioner import GenePredMultiHMMTransitioner
    b, L, q = 2, 400, 43
    g = torch.Generator().manual_seed(14)
    cls = torch.softmax(2 * torch.randn((1, b, L, 15), generator=g), -1)
    nuc = torch.nn.functional.one_hot(torch.randint(0, 4, (1, b, L), generator=g), 5).float()
    x = torch.cat([cls, nuc], -1).to(DEV)
    em = GenePredHMMEmitter(**CODONS, num_copies=3)
    em.build((1, b, L, 15))
    tr = GenePredMultiHMMTransitioner(k=3, initial_exon_len=200, initial_intron_len=4500, initial_ir_len=10000)
    cell = HmmCell([q], 15, em, tr).to(DEV)
    layer = MsaHmmLayer(cell, use_prior=False)
    layer.build(x.shape)
    params = [p for p in layer.parameters() if p.requires_grad]
    assert params
    with torch.no_grad():                                     # the labels: the most probable state
        labels = layer.state_posterior_log_probs(x).argmax(-1)
    grads = {}
    for value in (1, 0):
        answer = _Answer(value)
        monkeypatch.setattr(engine.lib(), "hmm_posterior_grad_scan_pays", answer)
        for p in params:
            p.grad = None
        logp = layer.state_posterior_log_probs(x, training=True, no_loglik=no_loglik)
        loss = -torch.gather(logp, -1, labels[..., None]).sum() / (b * L)
        loss.backward()
        assert answer.asked == 1
        grads[value] = [None if p.grad is None else p.grad.detach().clone() for p in params]
    assert any(t is not None for t in grads[1])
    for s_, c_ in zip(grads[0], grads[1]):
        assert (s_ is None) == (c_ is None)
        if s_ is not None:
            assert bool(torch.isfinite(c_).all())
            assert float((s_ - c_).abs().max()) <= 1e-4 * float(s_.abs().max())
