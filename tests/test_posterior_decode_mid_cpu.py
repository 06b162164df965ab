"""hmm_posterior_decode_mid (fused posterior decoding, 17..64 states) without a device: the argument checks of the C
ABI in the order the header states, the workspace query, the typed symbols, posterior decoding of the two-copy gene
model on the layer's CPU path against the fp64 oracle, and — on the oracle alone — that the cases of
tests/test_posterior_decode_mid_gpu.py (tests/posterior_decode_mid_cases.py) leave no more than the allowed share of
positions inside the margin within which a label may legitimately differ."""
import ctypes

import numpy as np
import pytest
import torch

import posterior_decode_mid_cases as cases
import posterior_decode_ref as ref
from hmm_layer_amd import build as hbuild
from hmm_layer_amd import engine
from hmm_layer_amd.MsaHmmCell import HmmCell
from hmm_layer_amd.MsaHMMLayer import MsaHmmLayer
from oracle import textbook
from test_modules_cpu import DenseTransitioner, PassThroughEmitter

OP = engine.OP_POSTERIOR


@pytest.fixture(scope="module")
def lib():
    hbuild.build()
    return engine.lib()


def table(entries):
    return (ctypes.c_int * len(entries))(*entries)


def test_validation_order_without_device(lib):
    # shape, q outside 17..64, null pointers, the class table, then the workspace; nothing here reaches a HIP call
    p = 0x10000                                                                 # never dereferenced
    eps, big = 1e-16, 1 << 40
    k, b, L, q = 2, 3, 17, 29
    f = lib.hmm_posterior_decode_mid
    assert lib.hmm_posterior_decode_mid_max_states() == 64
    assert f(None, None, None, k, b, 0, q, eps, None, 0, None, None, None, None, 0, None) == -1
    assert f(None, None, None, k, 0, L, 16, eps, None, 0, None, None, None, None, 0, None) == -1
    assert f(None, None, None, 0, b, L, 65, eps, None, 0, None, None, None, None, 0, None) == -1
    for bad_q in (1, 16, 65, 4096):
        assert f(None, None, None, k, b, L, bad_q, eps, None, 0, None, None, None, None, 0, None) == -2, bad_q
    for hole in range(5):                                                       # A, pi, E, label, workspace
        a = [p, p, p, p, p]
        a[hole] = None
        assert f(a[0], a[1], a[2], k, b, L, q, eps, None, 0, a[3], None, None, a[4], big, None) == -3, hole
    for tab, C in ((table([0] * q), 0), (table([0] * q), 17), (table([0, 1, 2] + [3] * (q - 3)), 3), (None, q + 1),
                   (None, 16), (table([0, -1] + [0] * (q - 2)), 2)):
        assert f(p, p, p, k, b, L, q, eps, tab, C, p, None, None, p, 0, None) == -6, C
    need = lib.hmm_posterior_decode_mid_workspace_bytes(k, b, L, q)
    for tab, C in ((None, q), (table([i % 4 for i in range(q)]), 4)):           # conf, loglik, state_class may be NULL
        assert f(p, p, p, k, b, L, q, eps, tab, C, p, None, None, p, need - 1, None) == -4
        assert f(p, p, p, k, b, L, q, eps, tab, C, p, p, p, p + 1, big, None) == -4


def test_workspace_query(lib):
    query = lib.hmm_posterior_decode_mid_workspace_bytes
    for k, b, L, q in ((1, 1, 1, 17), (2, 3, 17, 29), (1, 5, 333, 32), (1, 2, 300, 33), (1, 97, 20, 43), (2, 3, 530, 64),
                      (1, 1024, 1000, 57)):
        post = lib.hmm_workspace_bytes(OP, k, b, L, q)
        need = query(k, b, L, q)
        # hmm_posterior's workspace, then the parking region (k b L q floats) at the next 256-byte boundary
        assert post > 0 and post + 4 * k * b * L * q <= need < post + 4 * k * b * L * q + 256, (k, b, L, q)
    for q in (1, 16, 65, 100):
        assert query(2, 3, 17, q) == 0, q
    assert query(0, 3, 17, 29) == 0 and query(2, 3, 0, 29) == 0


def test_symbols_are_typed(lib):
    assert set(engine.DECODE_MID_SIGNATURES) == {"hmm_posterior_decode_mid_max_states",
                                                 "hmm_posterior_decode_mid_workspace_bytes", "hmm_posterior_decode_mid"}
    for name, (restype, argtypes) in engine.DECODE_MID_SIGNATURES.items():
        assert name not in engine._SIGNATURES and name not in engine.DECODE_SIGNATURES
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes)
    assert lib.hmm_posterior_decode_mid_workspace_bytes.restype is ctypes.c_size_t
    assert lib.hmm_posterior_decode_max_states() == 16                          # the q <= 16 entry point keeps its limit


def test_layer_cpu_path_against_the_oracle():
    # the two-copy gene model (29 states) on the layer's CPU path: the recursion in fp64, returned as fp32, so a class
    # sum of n states is within n * 2^-24 of the oracle's and two classes closer than twice that may swap
    A, pi = cases.gene(29)
    rng = np.random.default_rng(5)
    E = cases.emissions(rng, 1, 3, 200, 29)
    g64, ll64 = textbook.posterior(A, pi, E[0])
    layer = MsaHmmLayer(HmmCell([29], 29, PassThroughEmitter(), DenseTransitioner(A, pi)), use_prior=False)
    classes = cases.gene_classes(29)
    for tab, C in ((None, None), (classes, 6), (torch.tensor(classes), None)):
        with torch.no_grad():
            label, conf, ll = layer.posterior_decode(torch.as_tensor(E), state_class=tab, num_classes=C)
        assert label.dtype == torch.uint8 and tuple(label.shape) == (1, 3, 200)
        assert conf.dtype == torch.float32 and tuple(conf.shape) == (1, 3, 200)
        assert ll.dtype == torch.float64 and tuple(ll.shape) == (1, 3)
        want, c64, margin = ref.decode(g64, None if tab is None else classes, 6)
        sure = margin > 2e-6
        print("positions within the margin: %d of %d" % ((~sure).sum(), sure.size))
        assert (~sure).mean() <= cases.MARGIN_CAP
        assert np.array_equal(label[0].numpy()[sure], want[sure])
        assert np.abs(conf[0].numpy() - c64).max() <= 2e-6
        assert np.all(np.abs(ll[0].numpy() - ll64) <= 1e-9 * np.abs(ll64))


def oracle_gamma(A, pi, E):
    return np.stack([textbook.posterior(A[m], pi[m], E[m])[0] for m in range(E.shape[0])])


@pytest.mark.parametrize("case", cases.class_cases(), ids=lambda c: c[0])
def test_class_map_cases_leave_few_positions_inside_the_margin(case):
    """What the device test may skip: on the fp64 oracle, the share of a case's positions whose two best classes are
    within 2 tol(n) of each other stays below the cap, for every shape the device test runs."""
    tag, name, q, tab, C, seed = case
    n = cases.largest_class(tab, C)
    for chunk, shape in cases.CLASS_SHAPES:
        A, pi, E = cases.class_inputs(case, shape)
        margin = ref.decode(oracle_gamma(A, pi, E), tab, C)[2]
        share = float((margin <= 2 * cases.tol(n)).mean())
        print("%s %s: n = %d, within 2 tol(n) = %.3g: %.5f" % (tag, shape, n, 2 * cases.tol(n), share))
        assert share <= cases.MARGIN_CAP, (tag, shape, share)


@pytest.mark.parametrize("case", cases.oracle_cases(), ids=lambda c: c[0])
def test_oracle_cases_leave_few_positions_inside_the_margin(case):
    tag, name, q, tab, C, seed = case
    n = 1 if tab is None else cases.largest_class(tab, C)
    A, pi, E = cases.oracle_inputs(case)
    margin = ref.decode(oracle_gamma(A, pi, E), tab, C)[2]
    share = float((margin <= 2 * n * cases.STATE_TOL).mean())
    print("%s: n = %d, within %.3g: %.5f" % (tag, n, 2 * n * cases.STATE_TOL, share))
    assert share <= cases.ORACLE_CAP, (tag, share)
