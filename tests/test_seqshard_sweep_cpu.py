"""The oracle sweep of the sequence-sharded posterior, the part that needs no device: the cases of
tests/seqshard_cases.py are certified on the fp64 restatement (tests/seqshard_ref.py) and the oracle alone, and the host
side of the three hmm_seqshard_* entry points is pinned (symbols, workspace query, argument checks in their order).

  A  every operator case is finite, no reference column is empty, and 4 e32 < 1e-4 (e32 = the error of the operator
     formed in float32 numpy): the limit max(4 e32, 1e-6) of the GPU test can never hide a wrong factor;
  B  RefBackend over every cut list reports phi = 0 or <= PHI_LIMIT / 4 and agrees with the unsharded oracle to 1e-6;
  C  the robust set stored in the cases module is what certify() derives, and it is large and mixed enough.
"""
import numpy as np
import pytest

from hmm_layer_amd import build as hbuild
from hmm_layer_amd import engine, seqshard
from oracle import params

import seqshard_cases as sc

OK, BAD_SHAPE, Q_UNSUPPORTED, NULL_POINTER, WORKSPACE, BAD_ARGUMENT = 0, -1, -2, -3, -4, -6
SYMBOLS = ("hmm_seqshard_workspace_bytes", "hmm_seqshard_reduce", "hmm_seqshard_posterior")


# ---- the cases ------------------------------------------------------------------------------------------------------
def test_models():
    assert sc.PHI_LIMIT == seqshard.PHI_LIMIT and sc.EPS == engine.EPS
    for name in sc.SWEEP_MODELS + sc.C_MODELS + ("d5@hot", "g15@hot"):
        A, pi = sc.model(name)
        assert A.dtype == pi.dtype == np.float32 and np.abs(A.sum(-1) - 1).max() <= 1e-6
        assert all(sc.primitive(a) for a in A), name
    for name in sc.C_NONPRIMITIVE:
        assert not sc.primitive(sc.model(name)[0][0]), name
    # the gene models sit inside the compiled topologies' edge sets (and use every edge)
    for name, ed in (("g7", params.edges_simple()), ("g15", params.edges_multi(1))):
        support = np.zeros_like(sc.model(name)[0][0], dtype=bool)
        support[ed[:, 0], ed[:, 1]] = True
        assert np.array_equal(sc.model(name)[0][0] > 0, support), name
    assert not np.array_equal(*sc.model("d15+d15b")[0])
    assert sc.model("g15@hot")[1][0].tolist() == [1.0] + [0.0] * 14


@pytest.mark.parametrize("name", sc.SWEEP_MODELS)
def test_operator_cases_carry_the_comparison(name):
    worst = (-1.0, "")
    for spec in sc.a_cases((name,)):
        E, ref = sc.a_build(spec), sc.a_reference(spec)
        q = E.shape[-1]
        assert np.isfinite(ref["op"]).all() and (ref["op"][..., :q, :q].max(-2) > 0).all(), sc.a_id(spec)
        assert np.isfinite(ref["e32"]) and sc.TOL_FACTOR * ref["e32"] < sc.TOL_CAP, (sc.a_id(spec), ref["e32"])
        assert sc.op_error(ref["op"], ref["ex"], ref["op"], ref["ex"], q) == 0.0
        if spec.variant == "dead":
            assert (E[..., q // 2] == 0).all()
        if spec.variant == "tiny" and spec.Ls == 1000:
            assert ref["ex"][..., :q].max() < -30000, sc.a_id(spec)
        worst = max(worst, (ref["e32"], sc.a_id(spec)))
    print("SSWEEP-A %s: worst e32 %.3e (%s)" % ((name,) + worst))


def test_operator_norm_sees_a_wrong_factor_and_a_wrong_exponent():
    spec = sc.ASpec("g15", 100, 0, "plain", 0)
    ref = sc.a_reference(spec)
    op, ex = ref["op"].copy(), ref["ex"].copy()
    op[0, 1, 3, 9] *= 1.001                                  # one entry of one improbable column
    assert sc.op_error(op, ex, ref["op"], ref["ex"], 15) > ref["limit"]
    op, ex = ref["op"].copy(), ref["ex"].copy()
    ex[0, 2, 9] += 1
    assert sc.op_error(op, ex, ref["op"], ref["ex"], 15) >= 0.5
    ex[0, 2, 9] -= 1
    op[0, 2, :, 9] *= 2.0                                    # the same operator, written with another exponent
    ex[0, 2, 9] -= 1
    assert sc.op_error(op, ex, ref["op"], ref["ex"], 15) == 0.0
    ex[0, 0, 15] = 77                                        # pad lane: no contract
    assert sc.op_error(op, ex, ref["op"], ref["ex"], 15) == 0.0


@pytest.mark.parametrize("name", sc.B_MODELS)
def test_benign_cases_reference_has_no_flags(name):
    A, pi = sc.model(name)
    for spec in sc.b_cases((name,)):
        E = sc.b_build(name, spec.L)
        g64, ll64 = sc.oracle(name, "b", spec.L)
        out, lls, phis = sc.ref_run(A, pi, E, list(spec.cuts))
        phi = np.sum(phis, axis=0)
        assert np.isfinite(out).all() and ((phi == 0) | (phi <= sc.PHI_LIMIT / 4)).all(), (sc.b_id(spec), phi)
        assert np.abs(out - g64).max() <= 1e-6, sc.b_id(spec)
        for ll in lls:
            assert np.abs(ll - ll64).max() <= 1e-9 * np.abs(ll64).max(), sc.b_id(spec)


# ---- section C: the robust set --------------------------------------------------------------------------------------
def test_hard_cases_robust_set():
    lay = sc.c_layout()
    n_all = n_robust = n_flagged = 0
    by_place = dict.fromkeys(sc.PLACEMENTS, 0)
    for name in sc.C_MODELS:
        E, _ = sc.c_build(name)
        assert E.shape == (1, len(lay), sc.C_L, sc.model(name)[0].shape[-1])
        flags, robust = sc.certify(name)
        got = dict(flagged=tuple(int(i) for i in np.flatnonzero(robust & flags)),
                   unflagged=tuple(int(i) for i in np.flatnonzero(robust & ~flags)))
        assert got == sc.ROBUST[name], name
        # the restatement itself keeps the invariant: unflagged sequences match the unsharded oracle
        A, pi = sc.model(name)
        out, lls, _ = sc.ref_run(A, pi, E, list(sc.C_CUTS))
        g64, ll64 = sc.oracle(name, "c")
        ok = ~flags
        assert np.abs(out[0][ok] - g64[0][ok]).max() <= 1e-6, name
        assert np.abs(lls[1][0][ok] - ll64[0][ok]).max() <= 1e-9 * np.abs(ll64).max()
        n_all += len(lay)
        n_robust += int(robust.sum())
        n_flagged += int((robust & flags).sum())
        for h, f, r in zip(lay, flags, robust):
            if h.kind == "run" and f and r:
                by_place[h.place] += 1
    print("SSWEEP-C hard %d robust %d flagged %d by placement %s" % (n_all, n_robust, n_flagged, by_place))
    assert 2 * n_robust >= n_all
    assert 3 * n_flagged >= n_robust and 3 * (n_robust - n_flagged) >= n_robust
    assert all(v >= 1 for v in by_place.values()), by_place


def test_nonprimitive_models_are_flagged_by_the_reference():
    for name in sc.C_NONPRIMITIVE:
        A, pi = sc.model(name)
        _, _, phis = sc.ref_run(A, pi, sc.c_build(name)[0], list(sc.C_CUTS))
        assert all(np.isposinf(p).all() for p in phis), name


# ---- section F: the host side ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    hbuild.build()
    return engine.lib()


def reduce_call(lib, k=1, b=2, Ls=300, q=15, R=2, seq_start=1, ptrs=(256,) * 4, ws=256, nbytes=None):
    """hmm_seqshard_reduce with placeholder device pointers: every call here returns before any HIP call."""
    A, E, op, ex = ptrs
    if nbytes is None:
        nbytes = lib.hmm_seqshard_workspace_bytes(k, b, Ls, q, R)
    return lib.hmm_seqshard_reduce(A, E, k, b, Ls, q, 1e-16, seq_start, R, op, ex, ws, nbytes, None)


def posterior_call(lib, k=1, b=2, Ls=300, q=15, R=2, r=0, seq_start=None, mode=0, ptrs=(256,) * 8, ws=256, nbytes=None):
    """hmm_seqshard_posterior likewise; ptrs = A, pi, E, all_ops, all_exps, out, loglik, phi_out."""
    A, pi, E, ops, exs, out, ll, phi = ptrs
    if nbytes is None:
        nbytes = lib.hmm_seqshard_workspace_bytes(k, b, Ls, q, R)
    seq_start = int(r == 0) if seq_start is None else seq_start
    return lib.hmm_seqshard_posterior(A, pi, E, k, b, Ls, q, 1e-16, seq_start, ops, exs, R, r, mode, out, ll, phi, ws,
                                      nbytes, None)


def test_symbols(lib):
    for name in SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.hmm_scan_max_states() == 16


def test_workspace_query(lib):
    need = lib.hmm_seqshard_workspace_bytes
    assert need(1, 1, 1, 1, 1) > 0 and need(1, 1, 1, 1, 1) % 256 == 0
    assert need(2, 3, 5000, 16, 4) > 0 and need(2, 3, 5000, 16, 4) % 256 == 0
    assert need(1, 1, 100, 17, 2) == 0 and need(1, 1, 100, 15, 0) == 0 and need(1, 0, 100, 15, 2) == 0
    sizes = [need(2, 3, 5000, 15, R) for R in (1, 2, 3, 8, 64, 1024)]
    assert sizes == sorted(sizes) and sizes[-1] > sizes[0]
    assert need(2, 3, 5000, 15, 2) > lib.hmm_workspace_bytes(engine.OP_POSTERIOR, 2, 3, 5000, 15)
    with engine.option(engine.OPT_CHUNK, 16):
        small = need(1, 2, 100000, 15, 2)
    with engine.option(engine.OPT_CHUNK, 512):
        large = need(1, 2, 100000, 15, 2)
    assert small > large


def test_reduce_error_codes_in_order(lib):
    none = (None,) * 4
    assert reduce_call(lib, q=17, b=0, R=0, ptrs=none, ws=None, nbytes=0) == Q_UNSUPPORTED   # q ahead of everything
    assert reduce_call(lib, R=0, b=0, ptrs=none, ws=None, nbytes=0) == BAD_ARGUMENT          # R ahead of the shape
    assert reduce_call(lib, R=-1) == BAD_ARGUMENT
    assert reduce_call(lib, b=0, ptrs=none, ws=None, nbytes=0) == BAD_SHAPE                  # shape ahead of pointers
    assert reduce_call(lib, k=0) == BAD_SHAPE and reduce_call(lib, Ls=0) == BAD_SHAPE and reduce_call(lib, q=0) == BAD_SHAPE
    assert reduce_call(lib, ptrs=none, ws=None, nbytes=0) == NULL_POINTER                    # pointers ahead of workspace
    for x in range(4):
        ptrs = [256] * 4
        ptrs[x] = None
        assert reduce_call(lib, ptrs=tuple(ptrs), nbytes=0) == NULL_POINTER
    assert reduce_call(lib, ws=None) == NULL_POINTER
    assert reduce_call(lib, nbytes=0) == WORKSPACE
    need = lib.hmm_seqshard_workspace_bytes(1, 2, 300, 15, 2)
    assert reduce_call(lib, nbytes=need - 1) == WORKSPACE
    assert reduce_call(lib, ws=256 + 8, nbytes=need + 256) == WORKSPACE                      # misaligned


def test_posterior_error_codes_in_order(lib):
    none = (None,) * 8
    assert posterior_call(lib, q=17, b=0, R=0, r=5, mode=9, ptrs=none, ws=None, nbytes=0) == Q_UNSUPPORTED
    assert posterior_call(lib, R=0, b=0, r=5, mode=9, ptrs=none, ws=None, nbytes=0) == BAD_ARGUMENT
    assert posterior_call(lib, b=0, r=5, mode=9, ptrs=none, ws=None, nbytes=0) == BAD_SHAPE  # shape ahead of r and mode
    assert posterior_call(lib, k=0) == BAD_SHAPE and posterior_call(lib, Ls=0) == BAD_SHAPE
    assert posterior_call(lib, q=0) == BAD_SHAPE
    for r in (-1, 2, 3):                                                                     # r outside 0..R-1
        assert posterior_call(lib, r=r, seq_start=0, ptrs=none, ws=None, nbytes=0) == BAD_ARGUMENT
    assert posterior_call(lib, r=0, seq_start=0, ptrs=none, ws=None, nbytes=0) == BAD_ARGUMENT    # seq_start <=> r == 0
    assert posterior_call(lib, r=1, seq_start=1, ptrs=none, ws=None, nbytes=0) == BAD_ARGUMENT
    for mode in (-1, 3):
        assert posterior_call(lib, mode=mode, ptrs=none, ws=None, nbytes=0) == BAD_ARGUMENT      # mode ahead of pointers
    assert posterior_call(lib, ptrs=none, ws=None, nbytes=0) == NULL_POINTER
    for x in range(6):                                                                       # A .. out
        ptrs = [256] * 8
        ptrs[x] = None
        assert posterior_call(lib, ptrs=tuple(ptrs), nbytes=0) == NULL_POINTER
    assert posterior_call(lib, ws=None) == NULL_POINTER
    # loglik and phi_out may be NULL: such a call gets as far as the workspace check
    assert posterior_call(lib, ptrs=(256,) * 6 + (None, None), nbytes=0) == WORKSPACE
    assert posterior_call(lib, r=1, nbytes=0) == WORKSPACE
    need = lib.hmm_seqshard_workspace_bytes(1, 2, 300, 15, 2)
    assert posterior_call(lib, nbytes=need - 1) == WORKSPACE
    assert posterior_call(lib, ws=256 + 8, nbytes=need + 256) == WORKSPACE


def test_python_entry_points_have_no_cpu_path(lib):
    import torch
    with pytest.raises(engine.EngineError):
        engine.seqshard_reduce(torch.zeros(1, 15, 15), torch.zeros(1, 2, 3, 15), True, 2)
    with pytest.raises(engine.EngineError):
        engine.seqshard_posterior(torch.zeros(1, 15, 15), torch.zeros(1, 15), torch.zeros(1, 2, 3, 15),
                                  torch.zeros(1, 2, 2, 16, 16), torch.zeros(1, 2, 2, 16, dtype=torch.int32), 0)
