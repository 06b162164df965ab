"""hmm_posterior_walk / hmm_posterior_decode_wide (posteriors and fused posterior decoding by a per-sequence walk,
65..256 states) without a device: the argument checks of the C ABI in the order the header states, the state and
workspace queries, the typed symbols, engine.posterior_walk's refusals, the five-copy layer's posterior decoding on the
CPU path, and — on the fp64 oracle alone — that the label cases of tests/test_posterior_walk_gpu.py
(tests/posterior_walk_cases.py) leave no more than the allowed share of positions inside the margin within which a
label may legitimately differ."""
import ctypes

import numpy as np
import pytest
import torch

import posterior_decode_ref as ref
import posterior_walk_cases as cases
from hmm_layer_amd import build as hbuild
from hmm_layer_amd import engine
from hmm_layer_amd.MsaHmmCell import HmmCell
from hmm_layer_amd.MsaHMMLayer import MsaHmmLayer, _posterior_probs_host
from test_modules_cpu import DenseTransitioner, PassThroughEmitter


@pytest.fixture(scope="module")
def lib():
    hbuild.build()
    return engine.lib()


def table(entries):
    return (ctypes.c_int * len(entries))(*entries)


def test_state_range(lib):
    assert lib.hmm_posterior_walk_min_states() == 65 and lib.hmm_posterior_walk_max_states() == 256


def test_walk_validation_order_without_device(lib):
    # shape, q outside 65..256, null pointers, the mode, then the workspace; nothing here reaches a HIP call
    p = 0x10000                                                                 # never dereferenced
    eps, big = 1e-16, 1 << 40
    k, b, L, q = 2, 3, 17, 71
    f = lib.hmm_posterior_walk
    assert f(None, None, None, k, b, 0, q, eps, 7, None, None, None, 0, None) == -1
    assert f(None, None, None, k, 0, L, 64, eps, 7, None, None, None, 0, None) == -1
    assert f(None, None, None, 0, b, L, 257, eps, 7, None, None, None, 0, None) == -1
    for bad_q in (1, 16, 64, 257, 4096):
        assert f(None, None, None, k, b, L, bad_q, eps, 7, None, None, None, 0, None) == -2, bad_q
    for hole in range(5):                                                       # A, pi, E, out, workspace
        a = [p, p, p, p, p]
        a[hole] = None
        assert f(a[0], a[1], a[2], k, b, L, q, eps, 7, a[3], None, a[4], big, None) == -3, hole
    for mode in (-1, 3, 7):
        assert f(p, p, p, k, b, L, q, eps, mode, p, None, p, 0, None) == -6, mode
    need = lib.hmm_posterior_walk_workspace_bytes(k, b, L, q)
    for mode in (0, 1, 2):                                                      # loglik may be NULL
        assert f(p, p, p, k, b, L, q, eps, mode, p, None, p, need - 1, None) == -4
        assert f(p, p, p, k, b, L, q, eps, mode, p, p, p + 1, big, None) == -4


def test_decode_validation_order_without_device(lib):
    p = 0x10000
    eps, big = 1e-16, 1 << 40
    k, b, L, q = 2, 3, 17, 71
    f = lib.hmm_posterior_decode_wide
    assert f(None, None, None, k, b, 0, q, eps, None, 0, None, None, None, None, 0, None) == -1
    assert f(None, None, None, 0, b, L, 300, eps, None, 0, None, None, None, None, 0, None) == -1
    for bad_q in (1, 16, 64, 257, 4096):
        assert f(None, None, None, k, b, L, bad_q, eps, None, 0, None, None, None, None, 0, None) == -2, bad_q
    for hole in range(5):                                                       # A, pi, E, label, workspace
        a = [p, p, p, p, p]
        a[hole] = None
        assert f(a[0], a[1], a[2], k, b, L, q, eps, None, 0, a[3], None, None, a[4], big, None) == -3, hole
    for tab, C in ((table([0] * q), 0), (table([0] * q), 17), (table([0, 1, 2] + [3] * (q - 3)), 3), (None, q + 1),
                   (None, 16), (table([0, -1] + [0] * (q - 2)), 2)):
        assert f(p, p, p, k, b, L, q, eps, tab, C, p, None, None, p, 0, None) == -6, C
    need = lib.hmm_posterior_decode_wide_workspace_bytes(k, b, L, q)
    for tab, C in ((None, q), (table([i % 4 for i in range(q)]), 4)):           # conf, loglik, state_class may be NULL
        assert f(p, p, p, k, b, L, q, eps, tab, C, p, None, None, p, need - 1, None) == -4
        assert f(p, p, p, k, b, L, q, eps, tab, C, p, p, p, p + 1, big, None) == -4
    assert f(p, p, p, 1, 1, 5, 256, eps, None, 256, p, None, None, p, 0, None) == -4     # labels 0..255 fit the byte


def test_workspace_queries(lib):
    walk, dec = lib.hmm_posterior_walk_workspace_bytes, lib.hmm_posterior_decode_wide_workspace_bytes
    for k, b, L, q in ((1, 1, 1, 65), (2, 3, 17, 71), (1, 5, 333, 128), (1, 2, 300, 129), (2, 3, 530, 256),
                      (1, 1024, 1000, 253)):
        w = walk(k, b, L, q)
        assert w > 0 and w == walk(k, b, 7 * L + 1, q), (k, b, L, q)              # no part grows with L
        assert dec(k, b, L, q) == (w + 255) // 256 * 256 + 4 * k * b * L * q, (k, b, L, q)
    for q in (1, 16, 64, 257, 1027):
        assert walk(2, 3, 17, q) == 0 and dec(2, 3, 17, q) == 0, q
    for query in (walk, dec):
        assert query(0, 3, 17, 71) == 0 and query(2, 0, 17, 71) == 0 and query(2, 3, 0, 71) == 0
    assert walk(1, 1024, 10000, 253) < 64 << 20


def test_pays_is_zero_outside_the_range(lib):
    for dims in ((1, 32, 10000, 64), (1, 32, 10000, 257), (0, 32, 10000, 71), (1, 32, 0, 71)):
        assert lib.hmm_posterior_walk_pays(*dims) == 0, dims
    # the measured rule (profiles/posterior_walk.json): every measured cell pays, 1 / 32 / 1024 sequences at 71..253
    # states; more than 1024 sequences per call were not measured
    for q in cases.STATES:
        for k, b in ((1, 1), (1, 32), (1, 1024), (2, 512), (3, 5)):
            assert lib.hmm_posterior_walk_pays(k, b, 10000, q) == 1, (k, b, q)
            assert lib.hmm_posterior_walk_pays(k, b, 130, q) == 1, (k, b, q)
        for k, b in ((1, 1025), (2, 513), (1, 4096)):
            assert lib.hmm_posterior_walk_pays(k, b, 10000, q) == 0, (k, b, q)


def test_symbols_are_typed(lib):
    assert set(engine.POSTERIOR_WALK_SIGNATURES) == {
        "hmm_posterior_walk_min_states", "hmm_posterior_walk_max_states", "hmm_posterior_walk_workspace_bytes",
        "hmm_posterior_walk_pays", "hmm_posterior_walk", "hmm_posterior_decode_wide_workspace_bytes",
        "hmm_posterior_decode_wide"}
    for name, (restype, argtypes) in engine.POSTERIOR_WALK_SIGNATURES.items():
        assert name not in engine._SIGNATURES and name not in engine.DECODE_MID_SIGNATURES
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes)


def test_wrapper_refuses_other_state_counts_and_modes(lib):
    for q in (16, 64, 257, 1027):
        with pytest.raises(ValueError, match="65..256"):
            engine.posterior_walk(torch.eye(q)[None], torch.ones(q) / q, torch.rand(1, 2, 5, q))
    with pytest.raises(ValueError, match="mode"):
        engine.posterior_walk(torch.eye(71)[None], torch.ones(71) / 71, torch.rand(1, 2, 5, 71), mode=3)
    with pytest.raises(engine.EngineError, match="HIP device"):                 # in range: there is no CPU path
        engine.posterior_walk(torch.eye(71)[None], torch.ones(71) / 71, torch.rand(1, 2, 5, 71))


def test_layer_cpu_path_is_unchanged_for_the_five_copy_model():
    q = 71
    A, pi = cases.mid.gene(q)
    rng = np.random.default_rng(6)
    E = torch.as_tensor(cases.emissions(rng, 1, 3, 120, q))
    layer = MsaHmmLayer(HmmCell([q], q, PassThroughEmitter(), DenseTransitioner(A, pi)), use_prior=False)
    gamma, ll = _posterior_probs_host(torch.as_tensor(A)[None], torch.as_tensor(pi)[None], E, layer.cell.epsilon)
    classes = cases.gene_classes(q)
    for tab, C in ((None, None), (classes, 6)):
        with torch.no_grad():
            label, conf, lld = layer.posterior_decode(E, state_class=tab, num_classes=C)
        want = engine.decode_posterior(gamma, tab, 6 if tab else q)
        assert label.dtype == torch.uint8 and torch.equal(label, want[0]) and torch.equal(conf, want[1])
        assert torch.equal(lld, ll)
        assert int(label.max()) > 0


@pytest.mark.parametrize("case", cases.class_cases(), ids=lambda c: c[0])
def test_class_map_cases_leave_few_positions_inside_the_margin(case):
    """What the device test may leave out: on the fp64 oracle, the share of a case's positions whose two best classes
    are within 2 tol(n) of each other stays below the cap, for every shape the device test runs."""
    from oracle import textbook
    tag, kind, q, tab, C, seed = case
    n = cases.largest_class(tab, C)
    for shape in cases.CLASS_SHAPES:
        A, pi, E = cases.class_inputs(case, shape)
        g64 = np.stack([textbook.posterior(A[m], pi[m], E[m])[0] for m in range(E.shape[0])])
        margin = ref.decode(g64, tab, C)[2]
        share = float((margin <= 2 * cases.tol(n)).mean())
        print("%s %s: n = %d, within 2 tol(n) = %.3g: %.5f" % (tag, shape, n, 2 * cases.tol(n), share))
        assert share <= cases.MARGIN_CAP, (tag, shape, share)


@pytest.mark.parametrize("case", cases.oracle_cases(), ids=lambda c: c[0])
def test_oracle_cases_leave_few_positions_inside_the_margin(case):
    tag, kind, q, tab, C, seed = case
    n = 1 if tab is None else cases.largest_class(tab, C)
    for shape in cases.ORACLE_SHAPES:
        g64 = cases.oracle_inputs(case, shape)[3]
        margin = ref.decode(g64, tab, C)[2]
        share = float((margin <= 2 * n * cases.STATE_TOL).mean())
        print("%s %s: n = %d, within %.3g: %.5f" % (tag, shape, n, 2 * n * cases.STATE_TOL, share))
        assert share <= cases.ORACLE_CAP, (tag, shape, share)
