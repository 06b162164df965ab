"""Sequence-sharded posteriors for 17 to 64 states without a device: the protocol's fp64 restatement at width 32 / 64
(tests/seqshard_mid_ref.py) against the unsharded fp64 oracle over lists of cuts — that the inputs of
tests/seqshard_mid_cases.py can carry the GPU comparison —, the verdicts on the hard inputs, the exchange over gloo,
and the host side of hmm_seqshard_mid_* through ctypes."""
import ctypes
import os
import re
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import seqshard_mid_cases as mcs
import seqshard_mid_ref as smr
from hmm_layer_amd import build as hbuild
from hmm_layer_amd import engine, seqshard, seqshard_mid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement carries the comparison -------------------------------------------------------------------------
@pytest.mark.parametrize("name", mcs.MODELS)
def test_restatement_equals_the_oracle_on_benign_batches(name):
    """gamma within 1e-6, log-likelihood within 1e-6 relative, phi <= 2e-7 on every cut list (measured on g29, g43, d17,
    d64: gamma 4.3e-8, log-likelihood 7e-8, phi 0)."""
    assert mcs.PHI_LIMIT == seqshard.PHI_LIMIT
    A, pi = mcs.model(name)
    E = mcs.b_build(name, mcs.B_L)
    g64, ll64 = mcs.oracle(name, mcs.B_L)
    q = A.shape[-1]
    assert smr.tile(q) in (32, 64) and all(smr.primitive(a) for a in A)
    for cuts in mcs.B_CUTS:
        assert cuts[0] == 0 and cuts[-1] == mcs.B_L and len(mcs.B_CUTS[-1]) == 9
        out, lls, phis = mcs.ref_run(A, pi, E, list(cuts))
        eg = float(np.abs(out - g64).max())
        el = max(float((np.abs(ll - ll64) / np.abs(ll64)).max()) for ll in lls)
        ph = float(np.sum(phis, axis=0).max())
        print("REF %s cuts %s gamma %.2e ll %.2e phi %.2e" % (name, cuts, eg, el, ph))
        assert eg <= 1e-6 and el <= 1e-6 and ph <= 2e-7
        for ll in lls:
            assert np.array_equal(ll, lls[0])                # every rank: the same log-likelihood


def test_restatement_pads_with_zeros_and_knows_the_modes():
    A, pi = mcs.model("g29")
    E = mcs.b_build("g29", mcs.B_L)[:, :, :40]
    At, Et = torch.from_numpy(np.array(A)), torch.from_numpy(np.array(E))
    op, ex = smr.RefBackend().reduce(At, Et, True, 1)
    assert op.shape == (1, 3, 32, 32) and ex.shape == (1, 3, 32)
    assert not op[..., 29:, :].any() and not op[..., :, 29:].any() and not ex[..., 29:].any()
    s = op[..., :29, :29].sum(-2)
    assert ((s >= 0.5 - 1e-6) & (s < 1)).all()
    res = [smr.RefBackend().posterior(At, torch.from_numpy(np.array(pi)), Et, op.unsqueeze(2), ex.unsqueeze(2), 0, m)
           for m in (0, 1, 2)]
    g, ll = res[0][0].numpy().astype(np.float64), res[0][1].numpy()
    assert np.abs(np.log(g) - res[1][0].numpy()).max() <= 1e-5
    assert np.abs(res[2][0].numpy() - res[1][0].numpy() - ll[..., None, None]).max() <= 1e-4
    assert [smr.tile(q) for q in (0, 16, 17, 32, 33, 64, 65)] == [0, 0, 32, 32, 64, 64, 0]


def test_primitivity_of_the_models():
    for name in mcs.MODELS:
        assert all(smr.primitive(a) for a in mcs.model(name)[0]), name
    for name in mcs.NONPRIMITIVE:
        assert not smr.primitive(mcs.model(name)[0][0]), name
    # twelve squarings are needed: a 64-cycle with one chord is primitive with exponent beyond 256
    P = np.roll(np.eye(64), 1, axis=1)
    P[0, 2] = 1.0
    S = P > 0
    for _ in range(8):
        S = (S.astype(np.int64) @ S.astype(np.int64)) > 0
    assert not S.all() and smr.primitive(P)


# ---- hard cases -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,state,cuts", mcs.C_CASES, ids=mcs.c_id)
def test_hard_cases_have_robust_verdicts(name, state, cuts):
    """Sequence 1: twenty positions emit from one state alone, one that is left after one step for certain.  Every
    verdict of the restatement is a factor 10 away from the limit, and the neighbours' phi is 0.  Where it flags the
    sequence (state 8 of g29, state 11 of g43: summed phi 0.24 .. 0.83) the cut result is off by 1e-3 .. 1e-1 from the
    oracle: what the flag is for.  Where it does not (state 10 of g43) the result is as good as a benign one."""
    out, phi, flags = mcs.c_reference(name, state, cuts)
    g64, _ = mcs.c_oracle(name, state)
    err = np.abs(out - g64).max(axis=(0, 2, 3))
    print("HARD %s state %d cuts %s phi %s err %s" % (name, state, cuts, phi, err))
    assert ((phi >= 10 * mcs.PHI_LIMIT) | (phi <= 0.1 * mcs.PHI_LIMIT)).all()
    assert list(flags) == [False, mcs.C_FLAGGED[(name, state)], False]
    assert phi[0] == 0 and phi[2] == 0
    assert err[0] <= 1e-6 and err[2] <= 1e-6
    if flags[1]:
        assert 0.1 <= phi[1] <= 1.0
        assert len(cuts) == 2 or err[1] >= 1e-4             # (one slab: the restatement IS the serial recursion)
    else:
        assert err[1] <= 1e-6


# ---- the exchange over gloo ---------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


GLOO_CUTS = (0, 44, mcs.C_L)


def _worker(rank, world, port, out):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    A, pi = mcs.model("g29")
    E = mcs.c_build("g29", 8)
    At, pit = torch.from_numpy(np.array(A)), torch.from_numpy(np.array(pi))
    slab = torch.from_numpy(np.array(E[:, :, GLOO_CUTS[rank]:GLOO_CUTS[rank + 1]]))
    got, ll, flag = seqshard.posterior(At, pit, slab, backend=smr.RefBackend())
    got0, ll0 = got.numpy().copy(), ll.numpy().copy()
    got, ll = seqshard.gather_flagged(At, pit, slab, got, ll, flag, root=world - 1, backend=smr.RefBackend())
    out[rank] = (got0, ll0, flag.numpy(), got.numpy(), ll.numpy())
    dist.destroy_process_group()


def test_two_unequal_slabs_over_gloo_29_states():
    A, pi = mcs.model("g29")
    E = mcs.c_build("g29", 8)
    g64, ll64 = mcs.c_oracle("g29", 8)
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    assert out[0][0].shape == (1, 3, 44, 29) and out[1][0].shape == (1, 3, 76, 29)
    got = np.concatenate([out[0][0], out[1][0]], axis=2)
    flags = out[0][2]
    assert flags.tolist() == [[False, True, False]] and np.array_equal(out[1][2], flags)
    benign = ~flags[0]
    assert np.abs(got[0][benign] - g64[0][benign]).max() <= 1e-6
    for r in range(2):
        assert np.abs(out[r][1][0] - ll64[0])[benign].max() <= 1e-9 * np.abs(ll64).max()
    fixed = np.concatenate([out[0][3], out[1][3]], axis=2)
    assert np.abs(fixed - g64).max() <= 1e-6                 # the flagged sequence too, after gather_flagged
    for r in range(2):
        assert np.abs(out[r][4] - ll64).max() <= 1e-9 * np.abs(ll64).max()


def test_backend_is_chosen_by_q():
    for q in (1, 16):
        assert type(seqshard.posterior_backend(q)) is seqshard.EngineBackend
    for q in (17, 29, 64):
        assert type(seqshard.posterior_backend(q)) is seqshard_mid.MidEngineBackend
    with pytest.raises(ValueError, match="64"):
        seqshard.posterior_backend(65)
    a, e = seqshard.stack_slab_operators([torch.zeros(1, 3, 64, 64)] * 4, [torch.zeros(1, 3, 64, dtype=torch.int32)] * 4)
    assert a.shape == (1, 3, 4, 64, 64) and e.shape == (1, 3, 4, 64) and a.is_contiguous()


# ---- the C ABI without a device -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    hbuild.build()
    return seqshard_mid.lib()


NAMES = ("hmm_seqshard_mid_max_states", "hmm_seqshard_mid_tile", "hmm_seqshard_mid_workspace_bytes",
         "hmm_seqshard_mid_reduce", "hmm_seqshard_mid_posterior")


def test_symbols_declared_exported_and_typed(lib):
    text = open(os.path.join(ROOT, "include", "hmm_engine.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(hmm_seqshard_mid[a-z_]*)\s*\(", text))
    assert declared == set(NAMES)
    raw = ctypes.CDLL(engine.LIB_PATH)
    assert set(seqshard_mid.SIGNATURES) == set(NAMES)
    for n in NAMES:
        assert hasattr(raw, n)
        restype, argtypes = seqshard_mid.SIGNATURES[n]
        assert getattr(lib, n).restype is restype and list(getattr(lib, n).argtypes) == list(argtypes)
        assert n not in engine._SIGNATURES
    assert lib.hmm_seqshard_mid_max_states() == 64 == seqshard_mid.max_states()
    assert [lib.hmm_seqshard_mid_tile(q) for q in (0, 16, 17, 32, 33, 64, 65)] == [0, 0, 32, 32, 64, 64, 0]
    assert [seqshard_mid.tile(q) for q in (0, 16, 17, 32, 33, 64, 65)] == [smr.tile(q) for q in (0, 16, 17, 32, 33, 64, 65)]
    assert lib.hmm_abi_version() == 3 == engine.ABI_VERSION


def test_the_16_state_family_is_unchanged(lib):
    p = 0x10000
    assert lib.hmm_scan_max_states() == 16
    assert lib.hmm_seqshard_reduce(p, p, 1, 3, 100, 17, 1e-16, 0, 2, p, p, p, 1 << 40, None) == -2
    assert lib.hmm_seqshard_posterior(p, p, p, 1, 3, 100, 17, 1e-16, 0, p, p, 2, 1, 0, p, p, p, p, 1 << 40, None) == -2
    assert lib.hmm_seqshard_workspace_bytes(1, 3, 100, 17, 2) == 0


def test_workspace_query(lib):
    ws = lib.hmm_seqshard_mid_workspace_bytes
    # every b and every Ls >= 1: no routing rule of hmm_posterior applies (more than 96 sequences, fewer than 256
    # positions at 33..64 states; a slab of one position)
    for dims in [(1, 1, 1, 17), (1, 3, 100, 29), (2, 5, 1513, 64), (1, 1, 1000000, 43), (3, 4, 17, 33), (1, 200, 40, 57),
                 (1, 3, 1, 64)]:
        sizes = [ws(*dims, R) for R in (1, 2, 3, 8, 64)]
        assert all(s > 0 and s % 256 == 0 for s in sizes), dims
        assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] < sizes[-1]
    QT = 64
    assert ws(1, 3, 1024, 43, 8) >= 3 * (1024 // 512) * QT * QT * 4          # the chunk operators
    assert ws(1, 3, 100, 65, 2) == 0 and ws(1, 3, 100, 16, 2) == 0 and ws(1, 3, 100, 0, 2) == 0    # q outside 17 .. 64
    assert ws(1, 3, 100, 29, 0) == 0                         # R < 1
    for dims in [(0, 3, 100, 29), (1, 0, 100, 29), (1, 3, 0, 29), (1 << 13, 1 << 12, 16, 29)]:
        assert ws(*dims, 2) == 0


def test_validation_order_without_device(lib):
    p = 0x10000                                              # never dereferenced
    big = 1 << 40
    red, post = lib.hmm_seqshard_mid_reduce, lib.hmm_seqshard_mid_posterior
    k, b, Ls, q, R = 1, 3, 100, 29, 2

    def reduce_(k=k, b=b, Ls=Ls, q=q, R=R, A=p, E=p, op=p, ex=p, ws=p, n=big, seq_start=0):
        return red(A, E, k, b, Ls, q, 1e-16, seq_start, R, op, ex, ws, n, None)

    def post_(k=k, b=b, Ls=Ls, q=q, R=R, r=1, seq_start=0, mode=0, A=p, pi=p, E=p, ops=p, exs=p, out=p, ll=p, phi=p, ws=p,
              n=big):
        return post(A, pi, E, k, b, Ls, q, 1e-16, seq_start, ops, exs, R, r, mode, out, ll, phi, ws, n, None)

    # 1. q > 64 first, q < 17 too; ahead of everything (R, the shape, r, null pointers)
    for bad_q in (65, 4096, 16, 1, 0, -1):
        assert reduce_(q=bad_q, R=0, b=0, A=None) == -2
        assert post_(q=bad_q, R=0, b=0, A=None, r=5, mode=9) == -2
    # 2. R < 1, ahead of the shape
    assert reduce_(R=0, b=0, A=None) == -6
    assert post_(R=0, b=0, A=None) == -6
    # 3. the shape (k * b > 2^24 included), ahead of r, the mode and null pointers
    for bad in (dict(k=0), dict(b=0), dict(Ls=0), dict(k=1 << 13, b=1 << 12)):
        assert reduce_(A=None, **bad) == -1
        assert post_(A=None, r=7, mode=9, **bad) == -1
    # 4. r outside 0 .. R-1, seq_start against r, the mode; ahead of null pointers
    assert post_(r=-1, A=None) == -6 and post_(r=2, A=None) == -6
    assert post_(r=1, seq_start=1, A=None) == -6 and post_(r=0, seq_start=0, A=None) == -6
    assert post_(mode=-1, A=None) == -6 and post_(mode=3, A=None) == -6
    assert post_(r=0, seq_start=1, A=None) == -3
    # 5. every required pointer, ahead of the workspace's size; loglik and phi_out may be NULL
    for name in ("A", "E", "op", "ex", "ws"):
        assert reduce_(n=0, **{name: None}) == -3
    for name in ("A", "pi", "E", "ops", "exs", "out", "ws"):
        assert post_(n=0, **{name: None}) == -3
    assert post_(n=0, ll=None, phi=None) == -4
    # 6. the workspace: 256 bytes short of the query, then misaligned
    need = lib.hmm_seqshard_mid_workspace_bytes(k, b, Ls, q, R)
    assert need > 256
    for fn in (reduce_, post_):
        assert fn(n=need - 256) == -4
        assert fn(ws=p + 1, n=big) == -4
    # every q of 17 .. 64, every b, a slab of one position
    for kw in (dict(q=17), dict(q=32), dict(q=33), dict(q=64), dict(q=57, b=500), dict(q=43, Ls=1)):
        assert reduce_(n=0, **kw) == -4 and post_(n=0, **kw) == -4


def test_host_wrappers_reject_what_the_engine_does_not_cover(lib):
    for q in (16, 65):
        A, pi, E = torch.zeros(1, q, q), torch.zeros(1, q), torch.zeros(1, 2, 8, q)
        with pytest.raises(engine.EngineError, match="HIP device"):
            seqshard_mid.reduce(A, E, True, 1)
        with pytest.raises(ValueError, match="17 <= q <= 64"):
            seqshard_mid._shapes(A, E, pi)
    with pytest.raises(ValueError, match="bad sequence-sharded"):
        seqshard_mid._ws((1, 2, 8, 29), 0, torch.device("cpu"))
