"""hmm_loglik_grad_scan: the log-likelihood gradients per chunk of the scan plan for every model of 17..64 states
(hmm_grad_scan.inc; rows of 32 lanes up to 32 states, of 64 above).  Needs an MI355X.

Oracle: oracle.textbook.loglik_grad / loglik in fp64, with the tolerances of tests/test_grad_gpu.py::check restated:
dA 2e-4 * max|g64| on present edges and |g64(no clamp mask) - g64| + 5e-3 * max|g64| on absent ones (see that module's
docstring), dpi 2e-4 * max, dE 2e-5 * max + 1e-4 * |entry|, loglik 1e-6 * |ll| + 2e-4.  Against the whole-sequence
sweeps of hmm_loglik_grad (OPT_PGCHUNK = 0): 1e-4 * max + 1e-7 per tensor, the figure of the 29-state test.

Shapes: a full row (32, 64 states) and one past it (33), both row widths, ragged last chunks (L / chunk =
700 / 32, 333 / 16, 2100 / 64, 97 / 16), odd numbers of chunks per wave pair (3 * 21, 5 * 7 chains of 32-lane rows),
several models; the compiled 29-state topology (the sparse reduce and its pad-lane marks) once."""
import ctypes

import numpy as np
import pytest
import torch

from hmm_layer_amd import engine
from oracle import textbook

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CODONS = dict(start_codons=[("ATG", 1.)], stop_codons=[("TAG", .34), ("TAA", .33), ("TGA", .33)],
              intron_begin_pattern=[("NGT", .99), ("NGC", .005), ("NAT", .005)],
              intron_end_pattern=[("AGN", .99), ("ACN", .01)])


def dev(x, dtype=torch.float32):
    return torch.as_tensor(np.asarray(x), dtype=dtype, device=DEV)


def rand_model(rng, q):
    A = rng.random((q, q)) ** 2 + 1e-2
    A /= A.sum(-1, keepdims=True)
    pi = rng.random(q) + 0.1
    pi /= pi.sum()
    return A.astype(np.float32), pi.astype(np.float32)


_GENE = {}


def gene_A(copies):
    """A of GenePredMultiHMMTransitioner(k = copies): 29 states for 2 copies, 43 for 3, 57 for 4."""
    if copies not in _GENE:
        from hmm_layer_amd.gene_pred_hmm_transitioner import GenePredMultiHMMTransitioner
        tr = GenePredMultiHMMTransitioner(k=copies, initial_exon_len=200, initial_intron_len=4500, initial_ir_len=10000)
        with torch.no_grad():
            _GENE[copies] = tr.make_A()[0].numpy().astype(np.float32)
    return _GENE[copies]


def run(fn, A, pi, E, w=None):
    out = fn(dev(A), dev(pi), dev(E), None if w is None else dev(w))
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def check_oracle(got, A, pi, E, w=None, tag=""):
    dA, dpi, dE, ll = got
    for m in range(E.shape[0]):
        wm = None if w is None else w[m]
        rA, rpi, rE = textbook.loglik_grad(A[m], pi[m], E[m], wm)
        rU = textbook.loglik_grad(A[m], pi[m], E[m], wm, clamp_adjoint=False)[0]
        assert np.isfinite(dA[m]).all() and np.isfinite(dE[m]).all() and np.isfinite(dpi[m]).all(), tag
        tolA = np.where(A[m] > 0, 2e-4 * np.abs(rA).max(), np.abs(rU - rA) + 5e-3 * np.abs(rA).max())
        errA, errE = np.abs(dA[m] - rA), np.abs(dE[m] - rE)
        print("%s model %d: dA err %.3g (max %.3g)  dpi err %.3g (max %.3g)  dE err %.3g (max %.3g)"
              % (tag, m, errA.max(), np.abs(rA).max(), np.abs(dpi[m] - rpi).max(), np.abs(rpi).max(), errE.max(),
                 np.abs(rE).max()))
        assert np.all(errA <= tolA), (tag, m, errA.max(), np.abs(rA).max())
        assert np.abs(dpi[m] - rpi).max() <= 2e-4 * np.abs(rpi).max(), (tag, m)
        assert np.all(errE <= 2e-5 * np.abs(rE).max() + 1e-4 * np.abs(rE)), (tag, m, errE.max(), np.abs(rE).max())
        ll64 = textbook.loglik(A[m], pi[m], E[m])
        assert np.all(np.abs(ll[m] - ll64) <= 1e-6 * np.abs(ll64) + 2e-4), (tag, m)


def sweeps(A, pi, E, w=None):
    """hmm_loglik_grad's whole-sequence sweeps."""
    with engine.option(engine.OPT_PGCHUNK, 0):
        return run(engine.loglik_grad, A, pi, E, w)


MODELS = [(q, "dense") for q in (17, 24, 32, 33, 43, 57, 64)] + [(43, "gene"), (57, "gene")]
SHAPES = [(2, 700, 0), (3, 333, 16), (1, 2100, 64), (5, 97, 16)]
# the two-copy model: Scan32 with the compiled sparse reduce, whose marks k_pc_llselect reads from the pad lane
CASES = [(q, kind) + s for q, kind in MODELS for s in SHAPES] + [(29, "gene", 3, 333, 16)]


@pytest.mark.parametrize("q,kind,b,L,chunk", CASES)
def test_state_counts_and_widths(q, kind, b, L, chunk):
    rng = np.random.default_rng(1000 * q + L + b)
    if kind == "gene":
        A = gene_A({29: 2, 43: 3, 57: 4}[q])
        pi = (rng.random(q) + 0.1).astype(np.float32); pi /= pi.sum()
    else:
        A, pi = rand_model(rng, q)
    j = 20 % q
    E = (rng.random((1, b, L, q)) * 0.9 + 0.05).astype(np.float32)
    E[0, :, ::9, j] = 0.0                                      # clamped emissions: no gradient there
    w = (rng.random((1, b)) + 0.5).astype(np.float32)
    with engine.option(engine.OPT_CHUNK, chunk):
        got = run(engine.loglik_grad_scan, A[None], pi[None], E, w)
        n = engine.loglik_grad_scan_serial_count((1, b, L, q))
        assert L > engine.lib().hmm_loglik_grad_scan_chunk_len(1, b, L, q)      # more than one chunk
    check_oracle(got, A[None], pi[None], E, w, "q=%d %s b=%d L=%d" % (q, kind, b, L))
    assert n == 0
    assert np.all(got[2][0, :, ::9, j] == 0.0)
    for s_, c_ in zip(sweeps(A[None], pi[None], E, w), got):
        assert np.abs(s_ - c_).max() <= 1e-4 * np.abs(s_).max() + 1e-7


def test_several_models_in_one_call():
    """The gene model, a dense primitive model and a reducible one (block-diagonal A: the whole-sequence sweeps redo
    its sequences, masked, in the same call)."""
    rng = np.random.default_rng(43)
    q, b, L = 43, 3, 500
    Ad, pid = rand_model(rng, q)
    Ar = np.zeros((q, q), dtype=np.float32)
    Ar[:20, :20] = rand_model(rng, 20)[0]
    Ar[20:, 20:] = rand_model(rng, q - 20)[0]
    A = np.stack([gene_A(3), Ad, Ar])
    pi = np.stack([pid, pid, pid])
    E = (rng.random((3, b, L, q)) * 0.9 + 0.05).astype(np.float32)
    w = (rng.random((3, b)) + 0.5).astype(np.float32)
    got = run(engine.loglik_grad_scan, A, pi, E, w)
    assert engine.loglik_grad_scan_serial_count((3, b, L, q)) == b
    check_oracle(got, A, pi, E, w, "three models")
    ser = sweeps(A, pi, E, w)
    assert np.array_equal(got[2][2], ser[2][2]) and np.array_equal(got[0][2], ser[0][2])     # the redo IS the sweeps


def test_floor_decided_sequence_is_redone():
    """tests/test_grad_gpu.py::test_two_copy_model_floor_decided_sequence_is_redone on the 43-state gene model: a
    stretch where only one state emits, which the topology leaves after one step."""
    rng = np.random.default_rng(2)
    q, b, L = 43, 3, 900
    A = gene_A(3)
    pi = np.full(q, 1 / q, dtype=np.float32)
    E = (rng.random((1, b, L, q)) * 0.9 + 0.05).astype(np.float32)
    only = int(np.argmax((A > 0).sum(-1) == 1))              # a state with a single successor
    assert (A[only] > 0).sum() == 1
    E[0, 1, 400:420] = 0.0
    E[0, 1, 400:420, only] = 0.5
    auto = run(engine.loglik_grad_scan, A[None], pi[None], E)
    n = engine.loglik_grad_scan_serial_count((1, b, L, q))
    serial = sweeps(A[None], pi[None], E)
    assert 1 <= n <= b
    assert np.array_equal(auto[2][0, 1], serial[2][0, 1])
    check_oracle(auto, A[None], pi[None], E, None, "floor-decided")
    with engine.option(engine.OPT_PGCHUNK, 2):                # the hook: every sequence per chunk, no certificate
        run(engine.loglik_grad_scan, A[None], pi[None], E)
        assert engine.loglik_grad_scan_serial_count((1, b, L, q)) == 0


def raw_call(A, pi, E, w=None, want_ll=True, fill=float("nan"), name="hmm_loglik_grad_scan"):
    """The C entry point on sentinel-filled outputs -> numpy dA, dpi, dE, ll (None if not asked for)."""
    lib = engine.lib()
    k, b, L, q = E.shape
    A, pi, E = dev(A), dev(pi), dev(E)
    w = None if w is None else dev(w)
    ws = torch.empty(getattr(lib, name + "_workspace_bytes")(k, b, L, q), dtype=torch.uint8, device=DEV)
    dA = torch.full((k, q, q), fill, dtype=torch.float32, device=DEV)
    dpi = torch.full((k, q), fill, dtype=torch.float32, device=DEV)
    dE = torch.full((k, b, L, q), fill, dtype=torch.float32, device=DEV)
    ll = torch.full((k, b), fill, dtype=torch.float64, device=DEV) if want_ll else None
    rc = getattr(lib, name)(A.data_ptr(), pi.data_ptr(), E.data_ptr(), k, b, L, q, engine.EPS,
                            None if w is None else w.data_ptr(), dA.data_ptr(), dpi.data_ptr(), dE.data_ptr(),
                            None if ll is None else ll.data_ptr(), ws.data_ptr(), ws.numel(),
                            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, rc
    torch.cuda.synchronize()
    return [None if t is None else t.cpu().numpy() for t in (dA, dpi, dE, ll)]


@pytest.mark.parametrize("q", [24, 57])
def test_deterministic_and_everything_overwritten(q):
    rng = np.random.default_rng(q)
    b, L = 3, 333                                             # ragged last chunk
    A, pi = rand_model(rng, q)
    E = (rng.random((1, b, L, q)) * 0.9 + 0.05).astype(np.float32)
    w = (rng.random((1, b)) + 0.5).astype(np.float32)
    with engine.option(engine.OPT_CHUNK, 48):
        one = raw_call(A[None], pi[None], E, w)
        two = raw_call(A[None], pi[None], E, w, fill=-7.0)
    for x, y in zip(one, two):
        assert np.isfinite(x).all()                           # no sentinel left: dA, dpi, all of dE, loglik
        assert np.array_equal(x, y)
    assert not np.any(two[2] == -7.0) and not np.any(two[3] == -7.0)


def test_optional_arguments():
    rng = np.random.default_rng(5)
    q, b, L = 43, 2, 300
    A, pi = rand_model(rng, q)
    E = (rng.random((1, b, L, q)) * 0.9 + 0.05).astype(np.float32)
    full = raw_call(A[None], pi[None], E, np.ones((1, b), dtype=np.float32))
    bare = raw_call(A[None], pi[None], E, None, want_ll=False)
    for x, y in zip(full[:3], bare[:3]):
        assert np.array_equal(x, y)


ROUTING_SHAPES = [(1, 2, 4000, 43), (1, 2, 4000, 24), (1, 2, 4000, 64), (1, 1, 20000, 43), (1, 1, 20000, 24)]


def test_wrapper_routing():
    """engine.loglik_grad takes hmm_loglik_grad_scan exactly where hmm_loglik_grad_scan_pays says so."""
    lib = engine.lib()
    pays = [d for d in ROUTING_SHAPES if lib.hmm_loglik_grad_scan_pays(*d)]
    # where the rule says no — here: a single chunk — the wrapper is hmm_loglik_grad itself
    rng = np.random.default_rng(6)
    q, b, L = 43, 2, 40
    assert not lib.hmm_loglik_grad_scan_pays(1, b, L, q)
    A, pi = rand_model(rng, q)
    E = (rng.random((1, b, L, q)) * 0.9 + 0.05).astype(np.float32)
    for x, y in zip(run(engine.loglik_grad, A[None], pi[None], E), raw_call(A[None], pi[None], E, name="hmm_loglik_grad")):
        assert np.array_equal(x, y)
    if not pays:
        pytest.skip("hmm_loglik_grad_scan_pays is 0 for every shape of the list: see DESIGN 11c")
    k, b, L, q = pays[0]
    A, pi = rand_model(rng, q)
    E = (rng.random((k, b, L, q)) * 0.9 + 0.05).astype(np.float32)
    for x, y in zip(run(engine.loglik_grad, A[None], pi[None], E), run(engine.loglik_grad_scan, A[None], pi[None], E)):
        assert np.array_equal(x, y)
    # ... and differs from the sweeps in rounding only
    for s_, c_ in zip(sweeps(A[None], pi[None], E), run(engine.loglik_grad, A[None], pi[None], E)):
        assert np.abs(s_ - c_).max() <= 1e-4 * np.abs(s_).max() + 1e-7


def test_three_copy_layer_trains_the_same_either_way():
    """MsaHmmLayer.forward under autograd on the 43-state model: the parameter gradients with the routing left to the
    rule equal those of the whole-sequence sweeps."""
    from hmm_layer_amd.MsaHmmCell import HmmCell
    from hmm_layer_amd.MsaHMMLayer import MsaHmmLayer
    from hmm_layer_amd.gene_pred_hmm_emitter import GenePredHMMEmitter
    from hmm_layer_amd.gene_pred_hmm_transitioner import GenePredMultiHMMTransitioner
    b, L = 2, 400
    g = torch.Generator().manual_seed(14)
    cls = torch.softmax(2 * torch.randn((1, b, L, 15), generator=g), -1)
    nuc = torch.nn.functional.one_hot(torch.randint(0, 4, (1, b, L), generator=g), 5).float()
    x = torch.cat([cls, nuc], -1).to(DEV)
    em = GenePredHMMEmitter(**CODONS, num_copies=3)
    em.build((1, b, L, 15))
    tr = GenePredMultiHMMTransitioner(k=3, initial_exon_len=200, initial_intron_len=4500, initial_ir_len=10000)
    cell = HmmCell([43], 15, em, tr).to(DEV)
    layer = MsaHmmLayer(cell, use_prior=False)
    layer.build(x.shape)
    params = [p for p in layer.parameters() if p.requires_grad]
    assert params
    grads = {}
    for how in (engine.get_option(engine.OPT_PGCHUNK), 0):
        with engine.option(engine.OPT_PGCHUNK, how):
            for p in params:
                p.grad = None
            loglik, _ = layer(x, training=True)
            loglik.sum().backward()
            grads[how] = [None if p.grad is None else p.grad.detach().clone() for p in params]
    assert len(grads) == 2                                    # the default is not 0
    (ga, gb) = grads.values()
    assert any(t is not None for t in ga)
    for s_, c_ in zip(gb, ga):
        assert (s_ is None) == (c_ is None)
        if s_ is not None:
            assert bool(torch.isfinite(c_).all())
            assert float((s_ - c_).abs().max()) <= 1e-4 * float(s_.abs().max())
