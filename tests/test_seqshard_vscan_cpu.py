"""Sequence-sharded Viterbi for up to 64 states without a device: the protocol's int64 restatement at width 32 / 64
(tests/seqshard_vscan_ref.py) against the serial oracle over lists of cuts and over gloo, and the host side of
hmm_seqshard_vscan_* through ctypes."""
import contextlib
import ctypes
import os
import re
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import seqshard_vscan_ref as svr
from hmm_layer_amd import build as hbuild
from hmm_layer_amd import engine, seqshard, seqshard_vscan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = 57
# one slab; a single-position slab in front, in the middle, at the end; unequal slabs
CUTS = {"none": (0, L), "front1": (0, 1, L), "mid1": (0, 30, 31, L), "end1": (0, 56, L), "16_33": (0, 16, 33, L)}


def _ref_rank(r):
    return svr.RefVscanBackend(), contextlib.nullcontext()


@pytest.mark.parametrize("cut", sorted(CUTS))
@pytest.mark.parametrize("kind", svr.KINDS)
@pytest.mark.parametrize("q", [1, 16, 17, 29, 32, 33, 43, 64])
def test_protocol_equals_serial_oracle(q, kind, cut):
    logA, logpi, logE = svr.build(kind, 1, 2, L, q)
    want_path, want_score = svr.oracle_run(logA, logpi, logE)
    got = svr.run_cuts(_ref_rank, logA, logpi, logE, CUTS[cut])
    assert np.array_equal(got["path"], want_path)
    for s in got["scores"]:
        assert np.array_equal(s, want_score)
    QT = svr.tile(q)
    for vop, vbase, org in zip(got["vops"], got["vbases"], got["origins"]):
        assert vop.shape == (1, 2, QT, QT) and vbase.shape == (1, 2, QT) and org.shape == (1, 2, QT)
        assert not vop[..., :q, :q].max(-2).any()           # every column has maximum 0
    if kind == "flat":
        assert not got["path"].any()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


GLOO_CUT = (0, 20, L)                                        # unequal slabs


def _worker(rank, world, port, logA, logpi, logE, out):
    from hmm_layer_amd import seqshard
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    slab = logE[:, :, GLOO_CUT[rank]:GLOO_CUT[rank + 1]].contiguous()
    path, score = seqshard.viterbi(logA, logpi, slab, backend=svr.RefVscanBackend())
    out[rank] = (path.numpy(), score.numpy())
    dist.destroy_process_group()


def test_seqshard_viterbi_over_gloo_unequal_slabs_29_states():
    logA, logpi, logE = svr.build("random", 2, 3, L, 29)
    want_path, want_score = svr.oracle_run(logA, logpi, logE)
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_worker, args=(2, _free_port(), torch.from_numpy(logA), torch.from_numpy(logpi), torch.from_numpy(logE), out),
             nprocs=2, join=True)
    assert np.array_equal(np.concatenate([out[0][0], out[1][0]], axis=2), want_path)
    assert out[0][0].dtype == np.int32 and out[0][0].shape == (2, 3, 20)
    for r in range(2):
        assert np.array_equal(out[r][1], want_score)


def test_backend_is_chosen_by_q():
    for q in (1, 16):
        assert type(seqshard.viterbi_backend(q)) is seqshard.ViterbiEngineBackend
    for q in (17, 29, 64):
        assert type(seqshard.viterbi_backend(q)) is seqshard_vscan.VscanEngineBackend
    with pytest.raises(ValueError, match="64"):
        seqshard.viterbi_backend(65)


# ---- the C ABI without a device -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    hbuild.build()
    return seqshard_vscan.lib()


NAMES = ("hmm_seqshard_vscan_max_states", "hmm_seqshard_vscan_tile", "hmm_seqshard_vscan_workspace_bytes",
         "hmm_seqshard_vscan_reduce", "hmm_seqshard_vscan_apply", "hmm_seqshard_vscan_path")


def test_symbols_declared_exported_and_typed(lib):
    text = open(os.path.join(ROOT, "include", "hmm_engine.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(hmm_seqshard_vscan[a-z_]*)\s*\(", text))
    assert declared == set(NAMES)
    raw = ctypes.CDLL(engine.LIB_PATH)
    assert set(seqshard_vscan.SIGNATURES) == set(NAMES)
    for n in NAMES:
        assert hasattr(raw, n)
        restype, argtypes = seqshard_vscan.SIGNATURES[n]
        assert getattr(lib, n).restype is restype and list(getattr(lib, n).argtypes) == list(argtypes)
        assert n not in engine._SIGNATURES
    assert lib.hmm_seqshard_vscan_max_states() == lib.hmm_viterbi_scan_max_states() == 64
    assert [lib.hmm_seqshard_vscan_tile(q) for q in (0, 1, 32, 33, 64, 65)] == [0, 32, 32, 64, 64, 0]
    assert seqshard_vscan.max_states() == 64 and seqshard_vscan.tile(33) == 64
    assert lib.hmm_abi_version() == 3


def test_the_16_state_family_is_unchanged(lib):
    p = 0x10000
    assert lib.hmm_seqshard_viterbi_max_states() == 16
    assert lib.hmm_seqshard_viterbi_reduce(p, p, p, 1, 3, 100, 17, 0, 2, p, p, p, 1 << 40, None) == -2
    assert lib.hmm_seqshard_viterbi_workspace_bytes(1, 3, 100, 17, 2) == 0


def test_workspace_query(lib):
    ws = lib.hmm_seqshard_vscan_workspace_bytes
    for dims in [(1, 1, 1, 1), (1, 3, 100, 29), (2, 5, 1513, 64), (1, 1, 1000000, 43), (3, 4, 17, 17), (1, 2, 40, 16)]:
        sizes = [ws(*dims, R) for R in (1, 2, 3, 8, 64)]
        assert all(s > 0 and s % 256 == 0 for s in sizes)
        assert all(a <= b for a, b in zip(sizes, sizes[1:]))
        assert sizes[0] > lib.hmm_viterbi_scan_workspace_bytes(*dims)       # the plan's, plus entering scores and hops
    assert ws(1, 64, 1024, 29, 1) >= 64 * 64 * 1024          # backpointers: 64 bytes per position of a sequence
    assert ws(2, 7, 300, 43, 3) >= 64 * 2 * 7 * 300          # all k models at once
    assert ws(1, 3, 100, 65, 2) == 0                         # q > 64
    assert ws(1, 3, 100, 29, 0) == 0                         # R < 1
    for dims in [(0, 3, 100, 29), (1, 0, 100, 29), (1, 3, 0, 29), (1, 3, 100, 0), (1 << 13, 1 << 12, 16, 29)]:
        assert ws(*dims, 2) == 0


def test_validation_order_without_device(lib):
    p = 0x10000                                              # never dereferenced
    big = 1 << 40
    red, app, pth = lib.hmm_seqshard_vscan_reduce, lib.hmm_seqshard_vscan_apply, lib.hmm_seqshard_vscan_path
    k, b, Ls, q, R = 1, 3, 100, 29, 2

    def reduce_(k=k, b=b, Ls=Ls, q=q, R=R, A=p, pi=p, E=p, vop=p, vbase=p, ws=p, n=big, seq_start=0):
        return red(A, pi, E, k, b, Ls, q, seq_start, R, vop, vbase, ws, n, None)

    def apply_(k=k, b=b, Ls=Ls, q=q, R=R, r=1, seq_start=0, A=p, pi=p, E=p, vops=p, vbases=p, org=p, fin=p, sc=p, ws=p,
               n=big):
        return app(A, pi, E, k, b, Ls, q, seq_start, vops, vbases, R, r, org, fin, sc, ws, n, None)

    def path_(k=k, b=b, Ls=Ls, q=q, R=R, r=1, org=p, fin=p, path=p, ws=p, n=big):
        return pth(k, b, Ls, q, org, fin, R, r, path, ws, n, None)

    # 1. q > 64, ahead of everything (R, the shape, null pointers)
    assert reduce_(q=65, R=0, b=0, A=None) == -2
    assert apply_(q=65, R=0, b=0, A=None, r=5) == -2
    assert path_(q=65, R=0, b=0, org=None, r=5) == -2
    # 2. R < 1, ahead of the shape
    assert reduce_(R=0, b=0, A=None) == -6
    assert apply_(R=0, b=0, A=None) == -6
    assert path_(R=0, b=0, org=None) == -6
    # 3. the shape (k * b > 2^24 and more than 2^31 - 1 chunks included), ahead of r and of null pointers
    for bad in (dict(k=0), dict(b=0), dict(Ls=0), dict(q=0), dict(k=1 << 13, b=1 << 12),
                dict(k=1 << 12, b=1 << 12, Ls=1 << 30)):
        assert reduce_(A=None, **bad) == -1
        assert apply_(A=None, r=7, **bad) == -1
        assert path_(org=None, r=7, **bad) == -1
    # 4. r outside 0 .. R-1; apply: seq_start against r; ahead of null pointers
    assert apply_(r=-1, A=None) == -6 and apply_(r=2, A=None) == -6
    assert path_(r=-1, org=None) == -6 and path_(r=2, org=None) == -6
    assert apply_(r=1, seq_start=1, A=None) == -6 and apply_(r=0, seq_start=0, A=None) == -6
    assert apply_(r=0, seq_start=1, A=None) == -3
    # 5. every pointer, ahead of the workspace's size
    for name in ("A", "pi", "E", "vop", "vbase", "ws"):
        assert reduce_(n=0, **{name: None}) == -3
    for name in ("A", "pi", "E", "vops", "vbases", "org", "fin", "sc", "ws"):
        assert apply_(n=0, **{name: None}) == -3
    for name in ("org", "fin", "path", "ws"):
        assert path_(n=0, **{name: None}) == -3
    # 6. the workspace: 256 bytes short of the query, then misaligned
    need = lib.hmm_seqshard_vscan_workspace_bytes(k, b, Ls, q, R)
    assert need > 256
    for fn in (reduce_, apply_, path_):
        assert fn(n=need - 256) == -4
        assert fn(ws=p + 1, n=big) == -4
    # every q from 1 on is accepted
    assert reduce_(q=1, n=0) == -4 and reduce_(q=16, n=0) == -4 and reduce_(q=64, n=0) == -4


def test_host_wrappers_reject_what_the_engine_does_not_cover(lib):
    logA, logpi, logE = (torch.zeros(1, 65, 65), torch.zeros(1, 65), torch.zeros(1, 2, 8, 65))
    with pytest.raises(engine.EngineError, match="HIP device"):
        seqshard_vscan.reduce(logA, logpi, logE, True, 1)
    with pytest.raises(ValueError, match="64"):
        seqshard_vscan._ws((1, 2, 8, 65), 1, torch.device("cpu"))
    with pytest.raises(ValueError, match="bad sequence-sharded"):
        seqshard_vscan._ws((1, 2, 8, 29), 0, torch.device("cpu"))
