"""hmm_posterior_decode without a device: the argument checks of the C ABI in the order the header states, the host
wrapper's refusal of CPU tensors, and the semantics of posterior decoding pinned on the layer's CPU path against the
fp64 oracle (class sums in fp64, lowest maximal class, tests/posterior_decode_ref.py)."""
import ctypes

import numpy as np
import pytest
import torch

import posterior_decode_ref as ref
from hmm_layer_amd import build as hbuild
from hmm_layer_amd import engine
from hmm_layer_amd.MsaHmmCell import HmmCell
from hmm_layer_amd.MsaHMMLayer import MsaHmmLayer
from oracle import textbook
from test_layer_gpu import gene_setup
from test_modules_cpu import DenseTransitioner, PassThroughEmitter

# The layer's CPU posterior is the cell's recursion in fp64, returned as fp32: a class sum of at most n_max = 15 such
# values is within 15 * 2^-24 < 1e-6 of the oracle's, so two classes closer than 2e-6 may legitimately swap.
CPU_MARGIN = 2e-6


@pytest.fixture(scope="module")
def lib():
    hbuild.build()
    return engine.lib()


def table(entries):
    return (ctypes.c_int * len(entries))(*entries)


def test_validation_order_without_device(lib):
    # shape, q > 16, null pointers, the class table, then the workspace; nothing here reaches a HIP call
    p = 0x10000                                                                 # never dereferenced
    eps, big = 1e-16, 1 << 40
    k, b, L, q = 2, 3, 17, 7
    f = lib.hmm_posterior_decode
    assert lib.hmm_posterior_decode_max_states() == 16
    ident = (None, q)
    assert f(None, None, None, k, b, 0, q, eps, None, 0, None, None, None, None, 0, None) == -1
    assert f(None, None, None, k, 0, L, 17, eps, None, 0, None, None, None, None, 0, None) == -1
    assert f(None, None, None, k, b, L, 17, eps, None, 0, None, None, None, None, 0, None) == -2
    for hole in range(5):                                                       # A, pi, E, label, workspace
        a = [p, p, p, p, p]
        a[hole] = None
        assert f(a[0], a[1], a[2], k, b, L, q, eps, None, 0, a[3], None, None, a[4], big, None) == -3, hole
    for tab, C in ((table([0] * q), 0), (table([0] * q), 17), (table([0, 1, 2, 3, 3, 3, 3]), 3), (None, q + 1),
                   (table([0, -1, 0, 0, 0, 0, 0]), 2)):
        assert f(p, p, p, k, b, L, q, eps, tab, C, p, None, None, p, 0, None) == -6, C
    need = lib.hmm_workspace_bytes(engine.OP_POSTERIOR, k, b, L, q)
    assert need > 256
    for tab, C in (ident, (table([0, 1, 2, 3, 3, 3, 0]), 4)):                   # conf, loglik, state_class may be NULL
        assert f(p, p, p, k, b, L, q, eps, tab, C, p, None, None, p, need - 256, None) == -4
        assert f(p, p, p, k, b, L, q, eps, tab, C, p, p, p, p + 1, big, None) == -4


def test_symbols_are_typed(lib):
    for name, (restype, argtypes) in engine.DECODE_SIGNATURES.items():
        assert name not in engine._SIGNATURES
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes)


def test_host_wrapper_rejects_cpu_tensors(lib):
    A = torch.eye(3).unsqueeze(0)
    pi = torch.ones(3) / 3
    E = torch.rand(1, 2, 8, 3)
    with pytest.raises(engine.EngineError, match="HIP device"):
        engine.posterior_decode(A, pi, E)
    with pytest.raises(engine.EngineError, match="HIP device"):
        engine.posterior_decode(A, pi, E, state_class=[0, 1, 1])


def test_class_table_checks():
    assert engine.class_table(None, None, 5) == (None, 5)
    assert engine.class_table([0, 2, 1], None, 3) == ([0, 2, 1], 3)
    assert engine.class_table(torch.tensor([0, 0, 1], dtype=torch.int32), 4, 3) == ([0, 0, 1], 4)
    for bad in (([0, 1], None), ([0, 1, 2], 2), ([0, -1, 0], 2)):
        with pytest.raises(ValueError):
            engine.class_table(bad[0], bad[1], 3)
    with pytest.raises(ValueError):
        engine.class_table(None, 4, 3)


def layer_for(A, pi):
    q = A.shape[-1]
    return MsaHmmLayer(HmmCell([q], q, PassThroughEmitter(), DenseTransitioner(A, pi)), use_prior=False)


def test_layer_cpu_path_against_the_oracle():
    # the 15-state gene model with its emitter and transitioner on the CPU; the oracle gets the cell's own E
    cell, x, A, pi, _ = gene_setup(3, 333, seed=4, device="cpu")
    with torch.no_grad():
        E = cell.emission_probs(x, end_hints=None, training=False)[0].to(torch.float32).double().numpy()
    g64, ll64 = textbook.posterior(A, pi, E)
    layer = MsaHmmLayer(cell, use_prior=False)
    for tab, C in ((None, None), (ref.GENE_CLASSES, 5), (torch.tensor(ref.GENE_CLASSES), None)):
        with torch.no_grad():
            label, conf, ll = layer.posterior_decode(x, state_class=tab, num_classes=C)
        assert label.dtype == torch.uint8 and tuple(label.shape) == (1, 3, 333)
        assert conf.dtype == torch.float32 and tuple(conf.shape) == (1, 3, 333)
        assert ll.dtype == torch.float64 and tuple(ll.shape) == (1, 3)
        want, c64, margin = ref.decode(g64, None if tab is None else ref.GENE_CLASSES, 5)
        sure = margin > CPU_MARGIN
        print("positions within the margin: %d of %d" % ((~sure).sum(), sure.size))
        assert (~sure).mean() <= 0.01
        assert np.array_equal(label[0].numpy()[sure], want[sure])
        assert np.abs(conf[0].numpy() - c64).max() <= CPU_MARGIN
        assert np.all(np.abs(ll[0].numpy() - ll64) <= 1e-9 * np.abs(ll64))


def test_ties_go_to_the_lowest_class():
    q = 6
    A = np.full((q, q), 1 / q, dtype=np.float32)
    pi = np.full(q, 1 / q, dtype=np.float32)
    E = np.full((2, 40, q), 0.25, dtype=np.float32)
    layer = layer_for(A, pi)
    with torch.no_grad():
        for tab, C in ((None, None), ([0, 0, 1, 1, 2, 2], 3), ([2, 1, 0, 2, 1, 0], 3)):
            label, conf, _ = layer.posterior_decode(torch.as_tensor(E)[None], state_class=tab, num_classes=C)
            assert not label.any()
            assert np.allclose(conf.numpy(), 1 / q if tab is None else 1 / 3, rtol=1e-6)


def test_layer_is_inference_only():
    A = np.full((3, 3), 1 / 3, dtype=np.float32)
    layer = layer_for(A, np.full(3, 1 / 3, dtype=np.float32))
    E = torch.rand(1, 2, 8, 3, requires_grad=True)
    with pytest.raises(ValueError, match="state_posterior_log_probs"):
        layer.posterior_decode(E)
