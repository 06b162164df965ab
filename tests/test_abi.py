"""CPU-side checks of the drop-in boundary: the C-ABI library loads and exports exactly
what include/hmm_engine.h declares; host-side argument checking; no compute calls."""
import ctypes
import os
import re

import pytest
import torch

from hmm_layer_amd import build as hbuild
from hmm_layer_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    hbuild.build()
    return engine.lib()


def declared_functions():
    text = open(os.path.join(ROOT, "include", "hmm_engine.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(hmm_[a-z_]+)\s*\(", text)))


def test_header_symbols_are_exported(lib):
    names = declared_functions()
    assert {"hmm_forward", "hmm_backward", "hmm_posterior", "hmm_workspace_bytes"} <= set(names)
    raw = ctypes.CDLL(engine.LIB_PATH)
    for n in names:
        assert hasattr(raw, n), "symbol %s declared in hmm_engine.h is not exported" % n


def test_version_and_errors(lib):
    assert lib.hmm_abi_version() == engine.ABI_VERSION == 3
    assert lib.hmm_max_states() == 4096 and lib.hmm_scan_max_states() == 16
    assert lib.hmm_strerror(0) == b"ok"
    assert b"states" in lib.hmm_strerror(-2)


def test_plan_queries(lib):
    # chunk length is a multiple of 16, at most 1024, and the workspace grows with the op
    for dims in [(1, 4, 128, 3), (1, 256, 10000, 15), (1, 1024, 100000, 15), (2, 3, 17, 7)]:
        T = lib.hmm_chunk_len(*dims)
        assert T % 16 == 0 and 16 <= T <= 512
        w0 = lib.hmm_workspace_bytes(engine.OP_LOGLIK, *dims)
        w3 = lib.hmm_workspace_bytes(engine.OP_POSTERIOR, *dims)
        assert 0 < w0 <= w3
    assert lib.hmm_workspace_bytes(engine.OP_POSTERIOR, 1, 1024, 100000, 15) < 2 << 30
    assert lib.hmm_workspace_bytes(engine.OP_POSTERIOR, 1, 4, 128, 5000) == 0   # q unsupported
    assert lib.hmm_chunk_len(1, 4, 128, 5000) == -2
    assert lib.hmm_chunk_len(1, 4, 128, 1027) == 0                              # serial large-q path
    assert lib.hmm_workspace_bytes(engine.OP_POSTERIOR, 1, 4, 128, 1027) >= 3 * 4 * 1027 * 4
    assert lib.hmm_viterbi_workspace_bytes(1, 4, 128, 17) >= 4 * 128 * 64            # one wave per sequence
    assert lib.hmm_viterbi_workspace_bytes(1, 4, 128, 65) == 0 and lib.hmm_viterbi_max_states() == 64
    assert lib.hmm_chunk_len(1, 0, 128, 3) == -1


def test_null_and_shape_errors_without_device(lib):
    # argument validation happens before any HIP call
    assert lib.hmm_forward(None, None, None, 1, 1, 16, 3, 1e-16, None, None, None, 0, None) == -3
    assert lib.hmm_forward(None, None, None, 1, 1, 0, 3, 1e-16, None, None, None, 0, None) == -1
    assert lib.hmm_posterior(None, None, None, 1, 1, 16, 5000, 1e-16, 0, None, None, None, 0, None) == -2


@pytest.mark.parametrize("q", [15, 29, 48, 100])
def test_eps_outside_the_domain_is_refused(lib, q):
    # HMM_EPS_MIN = 1e-18 <= eps <= HMM_EPS_MAX = 1e-3 (include/hmm_engine.h): after the null pointers and the mode,
    # before the workspace; zero, negative and non-finite values are always outside.  Every other entry point that
    # takes eps: tests/test_eps_sweep_cpu.py::test_every_entry_point_refuses_eps_outside_the_domain
    p = 0x10000                                                                 # never dereferenced
    for eps in (0.0, -1e-16, float("nan"), float("inf"), 1e-20, 1e-30, 9.9e-19, 1.1e-3, 1.0):
        assert lib.hmm_forward(p, p, p, 1, 2, 300, q, eps, p, p, p + 1, 1 << 40, None) == -6
        assert lib.hmm_backward(p, p, 1, 2, 300, q, eps, p, p + 1, 1 << 40, None) == -6
        assert lib.hmm_posterior(p, p, p, 1, 2, 300, q, eps, 0, p, None, p + 1, 1 << 40, None) == -6
        assert lib.hmm_posterior(None, p, p, 1, 2, 300, q, eps, 0, p, None, p + 1, 1 << 40, None) == -3
    for eps in (1e-18, 1e-16, 1e-6, 1e-3):                                      # served: on to the workspace check
        assert lib.hmm_forward(p, p, p, 1, 2, 300, q, eps, p, p, p + 1, 1 << 40, None) == -4
        assert lib.hmm_backward(p, p, 1, 2, 300, q, eps, p, p + 1, 1 << 40, None) == -4
        assert lib.hmm_posterior(p, p, p, 1, 2, 300, q, eps, 0, p, None, p + 1, 1 << 40, None) == -4


def test_host_wrapper_rejects_cpu_tensors(lib):
    A = torch.eye(3).unsqueeze(0)
    pi = torch.ones(3) / 3
    E = torch.rand(1, 2, 8, 3)
    with pytest.raises(engine.EngineError, match="HIP device"):
        engine.posterior(A, pi, E)
    with pytest.raises(engine.EngineError, match="HIP device"):
        engine.forward(A, pi, E)


def test_missing_library_fails_loudly(monkeypatch):
    monkeypatch.setattr(engine, "_lib", None)
    monkeypatch.setattr(engine, "LIB_PATH", "/nonexistent/libhmm_engine.so")
    with pytest.raises(engine.EngineError, match="no CPU fallback"):
        engine.lib()


def test_midq_validation_order_without_device(lib):
    # 17..64 states: shape / q range, then null pointers, then the mode, then the workspace (null, size, alignment:
    # first against the serial plan, then with the chunked scan's region); nothing here reaches a HIP call
    p = 0x10000                                                                 # never dereferenced
    assert lib.hmm_forward(None, None, None, 1, 1, 300, 20, 1e-16, None, None, None, 0, None) == -3
    assert lib.hmm_forward(None, None, None, 1, 1, 0, 20, 1e-16, None, None, None, 0, None) == -1
    assert lib.hmm_backward(None, None, 1, 1, 300, 48, 1e-16, None, None, 0, None) == -3
    assert lib.hmm_posterior(None, None, None, 1, 1, 300, 48, 1e-16, 7, None, None, None, 0, None) == -3
    assert lib.hmm_posterior(p, p, p, 1, 1, 300, 48, 1e-16, 7, p, None, None, 0, None) == -6
    assert lib.hmm_posterior(p, p, p, 1, 1, 300, 48, 1e-16, 0, p, None, None, 0, None) == -3
    assert lib.hmm_posterior(p, p, p, 1, 1, 300, 48, 1e-16, 0, p, None, 0x10000, 256, None) == -4
    assert lib.hmm_posterior(p, p, p, 1, 1, 300, 20, 1e-16, 0, p, None, 0x10001, 1 << 30, None) == -4
    for q in (20, 48):
        assert lib.hmm_exact_count(engine.OP_POSTERIOR, 1, 1, 300, q, None, 0) == -3
    assert lib.hmm_exact_count(engine.OP_POSTERIOR, 1, 1, 100, 48, None, 0) == 0   # below the chunked path's minimum


# one shape per route: the 16-state scan plan (twice), both chunked widths, one wave per sequence (short sequences,
# and too many of them for the 64-state rows), the GEMM path
ROUTE_SHAPES = [(1, 1, 300, 15), (2, 3, 17, 7), (1, 1, 300, 20), (1, 1, 300, 48), (1, 1, 100, 48), (1, 2, 40, 100),
                (1, 200, 300, 48)]


@pytest.mark.parametrize("k,b,L,q", ROUTE_SHAPES)
def test_validation_order_on_every_route(lib, k, b, L, q):
    # the same precedence whichever path serves the shape: shape / q range, null pointers, the mode, then the
    # workspace (null, size, alignment); nothing here reaches a HIP call
    p = 0x10000                                                                 # never dereferenced
    eps = 1e-16
    big = 1 << 40
    assert lib.hmm_forward(p, p, p, k, b, 0, q, eps, p, p, p, big, None) == -1
    assert lib.hmm_forward(None, p, p, k, b, L, q, eps, p, p, p, big, None) == -3
    assert lib.hmm_forward(p, p, p, k, b, L, q, eps, p, p, None, big, None) == -3
    assert lib.hmm_backward(None, None, k, b, L, q, eps, None, None, 0, None) == -3
    assert lib.hmm_posterior(None, None, None, k, b, L, q, eps, 7, None, None, None, 0, None) == -3
    assert lib.hmm_posterior(p, p, p, k, b, L, q, eps, 7, p, None, p, big, None) == -6
    assert lib.hmm_posterior(p, p, p, k, b, L, q, eps, 0, p, None, None, big, None) == -3
    # 256 bytes short of what hmm_workspace_bytes asks for the same operation
    short = {op: lib.hmm_workspace_bytes(op, k, b, L, q) - 256
             for op in (engine.OP_LOGLIK, engine.OP_FORWARD, engine.OP_BACKWARD, engine.OP_POSTERIOR)}
    assert min(short.values()) > 0
    assert lib.hmm_forward(p, p, p, k, b, L, q, eps, None, p, p, short[engine.OP_LOGLIK], None) == -4
    assert lib.hmm_forward(p, p, p, k, b, L, q, eps, p, p, p, short[engine.OP_FORWARD], None) == -4
    assert lib.hmm_backward(p, p, k, b, L, q, eps, p, p, short[engine.OP_BACKWARD], None) == -4
    assert lib.hmm_posterior(p, p, p, k, b, L, q, eps, 0, p, None, p, short[engine.OP_POSTERIOR], None) == -4
    assert lib.hmm_posterior(p, p, p, k, b, L, q, eps, 0, p, None, p + 1, big, None) == -4


def test_midq_workspace_follows_the_chunked_path(lib):
    # 48 states, L = 300: up to 96 sequences take the chunked scan (the posterior adds its checkpoints), 97 do not
    w = {(op, b): lib.hmm_workspace_bytes(op, 1, b, 300, 48)
         for op in (engine.OP_LOGLIK, engine.OP_POSTERIOR) for b in (96, 97)}
    assert w[engine.OP_POSTERIOR, 96] > w[engine.OP_LOGLIK, 96]
    assert w[engine.OP_POSTERIOR, 97] == w[engine.OP_LOGLIK, 97]
    assert w[engine.OP_LOGLIK, 97] < w[engine.OP_LOGLIK, 96]


def test_missing_symbol_names_it(lib, monkeypatch):
    monkeypatch.setattr(engine, "_lib", None)
    monkeypatch.setitem(engine._SIGNATURES, "hmm_no_such_function", (ctypes.c_int, []))
    with pytest.raises(engine.EngineError, match="hmm_no_such_function"):
        engine.lib()
