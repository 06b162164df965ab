"""Host side of hmm_posterior_grad_scan (no device needed): the new symbols, limits, the chunk length and workspace
queries, the routing predicate and the argument checks in hmm_posterior_grad's order; and, from fp64 alone, that the
cases of tests/postgrad_scan_cases.py can carry the assertions of tests/test_posterior_grad_scan_gpu.py."""
import numpy as np
import pytest

from hmm_layer_amd import build as hbuild
from hmm_layer_amd import engine

import postgrad_scan_cases as sc

OK, BAD_SHAPE, Q_UNSUPPORTED, NULL_POINTER, WORKSPACE, BAD_ARGUMENT = 0, -1, -2, -3, -4, -6
SYMBOLS = ("hmm_posterior_grad_scan_max_states", "hmm_posterior_grad_scan_chunk_len", "hmm_posterior_grad_scan_pays",
           "hmm_posterior_grad_scan_workspace_bytes", "hmm_posterior_grad_scan_serial_count", "hmm_posterior_grad_scan")
PTRS = ("A", "pi", "E", "grad_out", "dA", "dpi", "dE")
CASES = sc.all_cases()


@pytest.fixture(scope="module")
def lib():
    hbuild.build()
    return engine.lib()


def call(lib, k=1, b=2, L=300, q=43, mode=engine.POST_LOG, ptrs=(256,) * 7, ws=256, nbytes=None):
    """hmm_posterior_grad_scan with placeholder device pointers: every call here returns before any HIP call."""
    A, pi, E, G, dA, dpi, dE = ptrs
    if nbytes is None:
        nbytes = lib.hmm_posterior_grad_scan_workspace_bytes(k, b, L, q)
    return lib.hmm_posterior_grad_scan(A, pi, E, k, b, L, q, 1e-16, mode, G, dA, dpi, dE, ws, nbytes, None)


def test_symbols_and_limits(lib):
    for name in SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.hmm_posterior_grad_scan_max_states() == 64
    assert lib.hmm_posterior_grad_max_states() == 64
    assert lib.hmm_abi_version() == 3 == engine.ABI_VERSION
    assert lib.hmm_set_option(9, 0) == BAD_ARGUMENT          # no new option


def test_workspace_query(lib):
    for dims in ((2, 3, 1000, 64), (1, 1, 1, 17), (1, 5, 97, 32), (1, 3, 333, 33)):
        n = lib.hmm_posterior_grad_scan_workspace_bytes(*dims)
        assert n > 0 and n % 256 == 0, dims
        k, b, L, q = dims
        assert n >= 3 * k * b * L * q * 4, dims                 # the two value arrays and the second part of dE
    assert lib.hmm_posterior_grad_scan_workspace_bytes(1, 1, 1, 65) == 0
    assert lib.hmm_posterior_grad_scan_workspace_bytes(1, 0, 1, 29) == 0
    big = (1, 64, 1000000, 64)                                # 64-bit sizes
    assert lib.hmm_posterior_grad_scan_workspace_bytes(*big) >= 3 * 64 * 1000000 * 64 * 4 > 2 ** 32
    for dims in ((2, 3, 1000, 15), (1, 1, 100000, 16), (1, 8, 40, 1)):      # q <= 16: hmm_posterior_grad's own plan
        assert lib.hmm_posterior_grad_scan_workspace_bytes(*dims) == lib.hmm_posterior_grad_workspace_bytes(*dims)
    with engine.option(engine.OPT_CHUNK, 16):                 # the chunk length sets the number of chunk operators
        small = lib.hmm_posterior_grad_scan_workspace_bytes(1, 1, 100000, 43)
    with engine.option(engine.OPT_CHUNK, 512):
        large = lib.hmm_posterior_grad_scan_workspace_bytes(1, 1, 100000, 43)
    assert small > large


def test_unsupported_shapes(lib):
    """L * q * 4 >= 2^31 - 4096 (32-bit row offsets) and k * b > 2^30 / 64: refused by every query and by the call."""
    assert 9000000 * 64 * 4 >= 2 ** 31 - 4096
    for dims in ((1, 1, 9000000, 64), (1, (1 << 24) + 1, 100, 43), ((1 << 12) + 1, 1 << 12, 100, 24)):
        assert lib.hmm_posterior_grad_scan_workspace_bytes(*dims) == 0, dims
        assert lib.hmm_posterior_grad_scan_chunk_len(*dims) == 0, dims
        assert lib.hmm_posterior_grad_scan_pays(*dims) == 0, dims
        assert call(lib, *dims, nbytes=1 << 50) == BAD_SHAPE, dims
        assert lib.hmm_posterior_grad_scan_serial_count(*dims, 256, 1 << 50) == BAD_SHAPE, dims
    assert lib.hmm_posterior_grad_scan_workspace_bytes(1, 1, 8000000, 64) > 0


def test_chunk_len(lib):
    for dims in ((1, 1, 100000, 29), (1, 1, 1000000, 43), (2, 1024, 100000, 57), (1, 5, 300, 64), (1, 32, 9999, 24),
                 (1, 3, 100, 17)):
        t = lib.hmm_posterior_grad_scan_chunk_len(*dims)
        assert t > 0 and t % 16 == 0 and t <= 512, (dims, t)
    assert lib.hmm_posterior_grad_scan_chunk_len(1, 1, 100, 65) == 0
    assert lib.hmm_posterior_grad_scan_chunk_len(1, 0, 100, 29) == 0
    with engine.option(engine.OPT_CHUNK, 48):
        assert lib.hmm_posterior_grad_scan_chunk_len(1, 1, 100000, 24) == 48
        assert lib.hmm_posterior_grad_scan_chunk_len(3, 7, 1000000, 64) == 48
    for c in CASES:                                           # the case shapes: more than one chunk
        with engine.option(engine.OPT_CHUNK, c.chunk):
            t = lib.hmm_posterior_grad_scan_chunk_len(1, c.b, c.L, c.q)
        assert 0 < t < c.L, sc.case_id(c)
        assert c.chunk == 0 or t == c.chunk, sc.case_id(c)


def test_pays_is_zero_where_the_question_does_not_arise(lib):
    for q in (1, 15, 16, 65, 100):
        assert lib.hmm_posterior_grad_scan_pays(1, 1, 1000000, q) == 0
    assert lib.hmm_posterior_grad_scan_pays(1, 0, 100, 43) == 0
    for q in (17, 24, 43, 57, 64):                             # below 4 chunks
        with engine.option(engine.OPT_CHUNK, 64):
            for L in (192, 65, 1):
                assert lib.hmm_posterior_grad_scan_chunk_len(1, 4, L, q) == 64
                assert lib.hmm_posterior_grad_scan_pays(1, 4, L, q) == 0
    # hmm_posterior_grad already runs the compiled 29-state topology per chunk at this shape
    with engine.option(engine.OPT_PGCHUNK, 0):
        whole = lib.hmm_posterior_grad_workspace_bytes(1, 32, 9999, 29)
    assert lib.hmm_posterior_grad_workspace_bytes(1, 32, 9999, 29) > whole      # (the chunk operators and maps)
    assert lib.hmm_posterior_grad_scan_pays(1, 32, 9999, 29) == 0
    with engine.option(engine.OPT_PGCHUNK, 0):                 # the whole-sequence sweeps are asked for
        for dims in ((1, 1, 100000, 43), (1, 4, 100000, 24), (1, 32, 9999, 64)):
            assert lib.hmm_posterior_grad_scan_pays(*dims) == 0


def test_pays_follows_the_measured_thresholds(lib):
    """rows of 32 lanes up to 128 sequences per call, rows of 64 up to 64, at 4 chunks or more."""
    for q, top in ((17, 128), (24, 128), (32, 128), (33, 64), (43, 64), (57, 64), (64, 64)):
        for k, b in ((1, 1), (1, 32), (1, top), (2, top // 2)):
            assert lib.hmm_posterior_grad_scan_pays(k, b, 9999, q) == 1, (q, k, b)
        for k, b in ((1, top + 1), (2, top // 2 + 1), (1, 512)):
            assert lib.hmm_posterior_grad_scan_pays(k, b, 9999, q) == 0, (q, k, b)
        assert lib.hmm_posterior_grad_scan_pays(1, 1, 100000, q) == 1
    assert lib.hmm_posterior_grad_scan_pays(1, 32, 9999, 29) == 0      # hmm_posterior_grad's own per-chunk path


def test_error_codes_in_hmm_posterior_grads_order(lib):
    none = (None,) * 7
    assert call(lib, q=65, ptrs=none, ws=None, nbytes=0) == Q_UNSUPPORTED      # q before pointers
    assert call(lib, b=0, ptrs=none, ws=None, nbytes=0) == BAD_SHAPE
    assert call(lib, b=0, q=65, ptrs=none, ws=None, nbytes=0) == BAD_SHAPE      # shape before q
    assert call(lib, k=0) == BAD_SHAPE and call(lib, L=0) == BAD_SHAPE and call(lib, q=0) == BAD_SHAPE
    assert call(lib, q=65, mode=7, ptrs=none, ws=None, nbytes=0) == Q_UNSUPPORTED      # q before the mode
    for q in (15, 24, 43):
        for name in ("hmm_posterior_grad_scan", "hmm_posterior_grad"):      # the same answers from both entry points
            def go(mode=engine.POST_LOG, ptrs=(256,) * 7, ws=256, nbytes=None):
                A, pi, E, G, dA, dpi, dE = ptrs
                if nbytes is None:
                    nbytes = getattr(lib, name + "_workspace_bytes")(1, 2, 300, q)
                return getattr(lib, name)(A, pi, E, 1, 2, 300, q, 1e-16, mode, G, dA, dpi, dE, ws, nbytes, None)
            assert go(mode=2, ptrs=none, ws=None, nbytes=0) == BAD_ARGUMENT     # the mode before pointers
            assert go(mode=engine.POST_LOG_NO_LL, ptrs=none, ws=None, nbytes=0) == BAD_ARGUMENT
            assert go(ptrs=none, ws=None, nbytes=0) == NULL_POINTER              # pointers before workspace
            for x in range(7):
                ptrs = [256] * 7
                ptrs[x] = None
                assert go(ptrs=tuple(ptrs), nbytes=0) == NULL_POINTER, PTRS[x]
            assert go(ws=None) == NULL_POINTER
            assert go(nbytes=0) == WORKSPACE
            need = getattr(lib, name + "_workspace_bytes")(1, 2, 300, q)
            assert go(nbytes=need - 1) == WORKSPACE
            assert go(ws=256 + 8, nbytes=need + 256) == WORKSPACE               # misaligned
    assert lib.hmm_posterior_grad_scan_serial_count(1, 0, 300, 43, None, 0) == BAD_SHAPE
    assert lib.hmm_posterior_grad_scan_serial_count(1, 2, 300, 65, None, 0) == Q_UNSUPPORTED
    assert lib.hmm_posterior_grad_scan_serial_count(1, 2, 300, 43, None, 0) == NULL_POINTER
    assert lib.hmm_posterior_grad_scan_serial_count(1, 2, 300, 43, 256, 0) == WORKSPACE


def test_python_entry_point_has_no_cpu_path(lib):
    import torch
    with pytest.raises(engine.EngineError):
        engine.posterior_grad_scan(torch.zeros(1, 43, 43), torch.zeros(1, 43), torch.zeros(1, 2, 3, 43),
                                   torch.zeros(1, 2, 3, 43))


# ---- the cases can carry their assertions (fp64 only) -------------------------------------------------------------
def test_case_list():
    ids = [sc.case_id(c) for c in CASES]
    assert len(set(ids)) == len(ids)
    for log in (False, True):
        mine = [c for c in CASES if c.log == log]
        for shape in sc.SHAPES:
            assert {(c.model, c.q) for c in mine if (c.b, c.L, c.chunk) == shape} >= \
                {("dense", q) for q in (17, 24, 32, 33, 48, 49, 64)} | {("gene", 43), ("gene", 57)}
        assert {(c.model, c.q) for c in mine if (c.b, c.L, c.chunk) == (2, 700, 0)} == \
            {("dense", 32), ("dense", 33), ("dense", 64), ("gene", 43)}
        assert [c for c in mine if (c.model, c.q, c.b, c.L, c.chunk) == ("gene", 43, 1, 2100, 64)]
        assert len([c for c in mine if c.q == 29]) == 1


@pytest.mark.parametrize("case", CASES, ids=sc.case_id)
def test_case_is_served_per_chunk_in_exact_arithmetic(case):
    """The model is primitive, and the per-chunk path's certificate is 100 x under its thresholds: F <= 1e-8 of
    EXACT_DELTA = 2e-6, and in log mode the exposed weight <= 1e-6 of PC_LOG_EXPOSED = 1e-4."""
    c = sc.build(case)
    A, pi, E, G = c["A"][0], c["pi"][0], c["E"][0], c["G"][0]
    q = case.q
    n = sc.primitive_power(A)
    assert n is not None and n <= q * q - 2 * q + 2, sc.case_id(case)
    assert np.all(pi > 1e-6)
    assert E.min() >= (0.0 if not case.log else 0.05) and E.max() <= 0.95
    if case.log:
        assert np.all(E > sc.EPS)                             # no holes
        assert np.all((G == 0) | (G == -1)) and np.all(G.sum(-1) <= -1)
    else:
        assert np.all(E[:, ::sc.HOLE_STEP, 20 % q] == 0.0) and (E <= sc.EPS).sum() == E[:, ::sc.HOLE_STEP, 20 % q].size
    F, exposed = sc.certificate(A, pi, E, G)
    print("PGSCAN-CPU %s primitive at %d  F <= %.2e  exposed <= %.2e" % (sc.case_id(case), n, F.max(), exposed.max()))
    assert F.max() <= 1e-8 <= sc.EXACT_DELTA / 100
    if case.log:
        assert exposed.max() <= 1e-6 <= sc.PC_LOG_EXPOSED / 100


@pytest.mark.parametrize("case", CASES, ids=sc.case_id)
def test_fine_norms_have_a_scale(case):
    """At most 5 % of a case's columns / rows fall under the small-scale rule of the fine norms (the cap of
    tests/test_postgrad_mid_cpu.py), and the oracle is finite and exactly 0 at the clamped emissions."""
    r = sc.reference(case)
    assert all(np.isfinite(x).all() for x in r["want"])
    for norm in sc.FINE_NORMS:
        print("PGSCAN-CPU %s %s e32 %.3e small %.3f" % (sc.case_id(case), norm, r["e32"][norm], r["small"][norm]))
        assert r["small"][norm] <= 0.05, (sc.case_id(case), norm)
    if not case.log:
        c = sc.build(case)
        assert np.all(r["want"][2][c["E"][0] <= sc.EPS] == 0.0)


@pytest.mark.parametrize("q", [43, 40])
def test_flagged_case_is_far_over_the_exposed_weight_rule(q):
    """Log mode with a dense upstream gradient: every sequence's exposed weight is >= 1e-3 of sum |G|, ten times
    PC_LOG_EXPOSED; the models are primitive, so the routing is the sequences'."""
    c = sc.flagged_case(q)
    assert sc.primitive_power(c["A"][0]) is not None
    F, exposed = sc.certificate(c["A"][0], c["pi"][0], c["E"][0], c["G"][0])
    print("PGSCAN-CPU flagged q=%d F %s exposed %s" % (q, F, exposed))
    assert np.all(exposed >= 1e-3) and 1e-3 >= 10 * sc.PC_LOG_EXPOSED
    assert F.max() <= 1e-8                                    # ... and not the certificate F


def test_floor_decided_case():
    """Sequence 1 is over the certificate by orders of magnitude, its neighbours 100 x under it and under the
    exposed-weight rule."""
    c = sc.floor_decided_case()
    assert sc.primitive_power(c["A"][0]) is not None
    F, exposed = sc.certificate(c["A"][0], c["pi"][0], c["E"][0], c["G"][0])
    print("PGSCAN-CPU floor-decided F %s exposed %s" % (F, exposed))
    assert F[1] >= 100 * sc.EXACT_DELTA
    for s in (0, 2):
        assert F[s] <= 1e-8 and exposed[s] <= 1e-6
