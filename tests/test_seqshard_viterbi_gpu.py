"""Sequence-sharded Viterbi on the engine (hmm_seqshard_viterbi_reduce / _apply / _path): ranks played one after
another on one GPU, one stream (hence one workspace) per rank; all reduces first, then all applies, then all paths, so
the workspaces have to survive.  Everything is compared with array_equal: against engine.viterbi on the uncut tensor,
against oracle/viterbi.py, and piece by piece against the int64 restatement (tests/seqshard_viterbi_ref.py).

Every log A here is the log of a seqshard_cases model (zeros -> -inf: absent edges), so "g7" / "g15" keep their compiled
topology whatever the input kind: "ties", "flat" and "absent" redraw the PRESENT edges only."""
import contextlib
import functools

import numpy as np
import pytest
import torch

import seqshard_cases as sc
import seqshard_viterbi_ref as svr
from hmm_layer_amd import build as hbuild
from hmm_layer_amd import engine, seqshard

pytestmark = pytest.mark.gpu

KINDS = svr.KINDS + ("einf", "ebig")
B_MODELS = ("d1", "d2", "d5", "d15", "d16", "g7", "g15", "g15+d15", "d15+d15b")
LONG_L, LONG_CUTS, LONG_MODELS = 1513, (0, 513, 1513), ("g7", "g15", "d16")


@pytest.fixture(scope="module", autouse=True)
def _built():
    hbuild.build()


def dev(x):
    return torch.as_tensor(np.array(x) if isinstance(x, np.ndarray) else x, device="cuda:0")     # (inputs are read-only)


@functools.lru_cache(maxsize=None)
def inputs(name, kind, b, L):
    """-> logA (k,q,q), logpi (k,q), logE (k,b,L,q) float32, read-only."""
    A, pi = sc.model(name)
    k, q = A.shape[:2]
    rng = np.random.default_rng([41, B_MODELS.index(name) if name in B_MODELS else 99, KINDS.index(kind), b, L])
    with np.errstate(divide="ignore"):
        logA, logpi = np.log(A).astype(np.float32), np.log(pi).astype(np.float32)
    logE = np.log(rng.random((k, b, L, q)) * 0.9 + 0.05).astype(np.float32)
    present = A > 0
    if kind == "ties":
        logA = np.where(present, -rng.integers(0, 3, A.shape), -np.inf).astype(np.float32)
        logpi = -rng.integers(0, 3, pi.shape).astype(np.float32)
        logE = -rng.integers(0, 3, logE.shape).astype(np.float32)
    elif kind == "flat":
        logA = np.where(present, -1.5, -np.inf).astype(np.float32)
        logpi, logE = np.full_like(logpi, -1.5), np.full_like(logE, -1.5)
    elif kind == "absent":
        logA = np.where(present & (rng.random(A.shape) >= 0.6), logA, -np.inf).astype(np.float32)
    elif kind == "einf":                                     # -inf entries, and whole rows of them
        logE[rng.random(logE.shape) < 0.1] = -np.inf
        logE[:, :, rng.integers(0, L, max(L // 20, 1))] = -np.inf
    elif kind == "ebig":                                     # above the clamp: Q() takes them as +1024
        m = rng.random(logE.shape)
        logE[m < 0.05] = 1500.0
        logE[m > 0.97] = np.inf
    return sc._frozen(logA, logpi, logE)


@functools.lru_cache(maxsize=None)
def oracle(name, kind, b, L):
    return sc._frozen(*svr.oracle_run(*inputs(name, kind, b, L)))


def unsharded(logA, logpi, logE):
    path, score = engine.viterbi(dev(logA), dev(logpi), dev(logE))
    return path.cpu().numpy(), score.cpu().numpy()


@functools.lru_cache(maxsize=None)
def rank_stream(r):
    return torch.cuda.Stream()                               # (kept: the engine caches one workspace per stream)


def engine_cuts(logA, logpi, logE, cuts):
    streams = [rank_stream(r) for r in range(len(cuts) - 1)]
    return svr.run_cuts(lambda r: (seqshard.ViterbiEngineBackend(), torch.cuda.stream(streams[r])), logA, logpi, logE,
                        cuts, dev=dev, sync=torch.cuda.synchronize)


def check_against(got, want_path, want_score, what):
    assert got["path"].dtype == np.int32
    assert np.array_equal(got["path"], want_path), what
    for r, s in enumerate(got["scores"]):
        assert np.array_equal(s, want_score), "%s: score on rank %d" % (what, r)


# ---- A: the slab operator alone -------------------------------------------------------------------------------------
A_MODELS = [("d1", 0), ("d2", 0), ("d16", 0), ("g7", 0), ("g15", 0), ("g7", 1), ("g15", 1)]
A_LENGTHS = {0: (1, 2, 15, 16, 17, 33, 100), 16: (496, 512, 513, 1000)}    # chunk 16: 31 / 32 / 33 / 63 chunks


@pytest.mark.parametrize("chunk", sorted(A_LENGTHS))
@pytest.mark.parametrize("name,force_dense", A_MODELS)
def test_a_slab_operator(name, force_dense, chunk):
    ref = svr.RefViterbiBackend()
    with engine.option(engine.OPT_CHUNK, chunk), engine.option(engine.OPT_FORCE_DENSE, force_dense):
        for b in (3, 5):                                     # four chains per wave: neither fills one
            for Ls in A_LENGTHS[chunk]:
                logA, logpi, logE = inputs(name, "random", b, Ls)
                q = logE.shape[-1]
                for seq_start in (0, 1):
                    vop, vbase = engine.seqshard_viterbi_reduce(dev(logA), dev(logpi), dev(logE), seq_start, 2)
                    vop, vbase = vop.cpu().numpy().astype(np.int64), vbase.cpu().numpy()
                    wop, wbase = (x.numpy().astype(np.int64) for x in ref.reduce(logA, logpi, logE, seq_start, 2))
                    what = "%s b=%d Ls=%d seq_start=%d" % (name, b, Ls, seq_start)
                    got = vop[..., :q, :q] + vbase[..., None, :q]
                    want = wop[..., :q, :q] + wbase[..., None, :q]
                    assert np.array_equal(got, want), what
                    assert np.array_equal(vop[..., :q, :q].max(-2), np.zeros_like(vbase[..., :q])), what
                    assert not vop[..., q:, :].any() and not vop[..., :, q:].any(), what


# ---- B: end to end --------------------------------------------------------------------------------------------------
B_REF_CUT = (0, 16, 33, 48, 117, sc.B_L)                     # the restatement's pieces are compared on this cut


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", B_MODELS)
def test_b_end_to_end(name, kind):
    logA, logpi, logE = inputs(name, kind, 3, sc.B_L)
    q = logE.shape[-1]
    want_path, want_score = oracle(name, kind, 3, sc.B_L)
    eng_path, eng_score = unsharded(logA, logpi, logE)
    assert np.array_equal(eng_path, want_path) and np.array_equal(eng_score, want_score)
    if kind == "flat" and name[0] == "d":
        assert not want_path.any()
    assert B_REF_CUT in sc.B_CUTS
    for cuts in sc.B_CUTS:
        got = engine_cuts(logA, logpi, logE, cuts)
        check_against(got, want_path, want_score, "%s %s cuts %s" % (name, kind, cuts))
        for f in got["finals"]:
            assert np.array_equal(f, want_path[:, :, -1])
        if cuts == B_REF_CUT:
            ref = svr.run_cuts(lambda r: (svr.RefViterbiBackend(), contextlib.nullcontext()), logA, logpi, logE, cuts)
            for r in range(len(cuts) - 1):
                g = got["vops"][r].astype(np.int64)[..., :q, :q] + got["vbases"][r][..., None, :q]
                w = ref["vops"][r].astype(np.int64)[..., :q, :q] + ref["vbases"][r][..., None, :q]
                assert np.array_equal(g, w), "operator of rank %d" % r
                assert np.array_equal(got["origins"][r][..., :q], ref["origins"][r][..., :q]), "map of rank %d" % r
                if r == 0:
                    assert not got["origins"][r].any()


# ---- C: two levels inside a slab ------------------------------------------------------------------------------------
@pytest.mark.parametrize("scan2", [0, 1])
@pytest.mark.parametrize("name", LONG_MODELS)
def test_c_two_levels_inside_a_slab(name, scan2):
    logA, logpi, logE = inputs(name, "random", 3, LONG_L)
    want_path, want_score = oracle(name, "random", 3, LONG_L)
    with engine.option(engine.OPT_CHUNK, 16), engine.option(engine.OPT_SCAN2, scan2):
        eng_path, eng_score = unsharded(logA, logpi, logE)
        got = engine_cuts(logA, logpi, logE, LONG_CUTS)     # 33 and 63 chunks of 16
    assert np.array_equal(eng_path, want_path) and np.array_equal(eng_score, want_score)
    check_against(got, want_path, want_score, "%s scan2=%d" % (name, scan2))


# ---- D: 64-bit bases across a cut -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def deep_inputs(name):
    logA, logpi, logE = inputs(name, "random", 3, LONG_L)
    logE = logE.copy()
    logE[:, :, 400:1201] = -np.inf                           # 801 positions at -2^26 each: the scores pass -2^31 in Q16
    return sc._frozen(logA, logpi, logE)


@pytest.mark.parametrize("scan2", [0, 1])
@pytest.mark.parametrize("name", LONG_MODELS)
def test_d_64_bit_bases_across_a_cut(name, scan2):
    logA, logpi, logE = deep_inputs(name)
    want_path, want_score = svr.oracle_run(logA, logpi, logE)
    assert (want_score * 65536 < -float(1 << 35)).all()
    with engine.option(engine.OPT_CHUNK, 16), engine.option(engine.OPT_SCAN2, scan2):
        eng_path, eng_score = unsharded(logA, logpi, logE)
        got = engine_cuts(logA, logpi, logE, LONG_CUTS)     # the cut at 513 lies inside the -inf stretch
    assert np.array_equal(eng_path, want_path) and np.array_equal(eng_score, want_score)
    check_against(got, want_path, want_score, "%s scan2=%d" % (name, scan2))
    for r in range(2):                                       # to the last bit
        assert np.array_equal(got["scores"][r].view(np.int64), want_score.view(np.int64))


# ---- E: R = 1 -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,L,chunk", [("g15", sc.B_L, 0), ("d5", sc.B_L, 0), ("g15+d15", LONG_L, 16), ("d16", 1, 0)])
def test_e_single_rank_equals_hmm_viterbi(name, L, chunk):
    kind = "random"
    logA, logpi, logE = inputs(name, kind, 3, L)
    with engine.option(engine.OPT_CHUNK, chunk):
        eng_path, eng_score = unsharded(logA, logpi, logE)
        runs = [engine_cuts(logA, logpi, logE, (0, L)) for _ in range(3)]
    want_path, want_score = oracle(name, kind, 3, L)
    assert np.array_equal(eng_path, want_path) and np.array_equal(eng_score, want_score)
    for got in runs:
        check_against(got, eng_path, eng_score, name)
        for key in ("vops", "vbases", "origins", "finals"):
            assert np.array_equal(got[key][0], runs[0][key][0]), key
        assert not got["origins"][0].any()


# ---- F: the layer-level wrapper -------------------------------------------------------------------------------------
def test_f_viterbi_sharded_forms_the_logs_as_viterbi_does(monkeypatch):
    """Viterbi.viterbi_sharded(E_slab, cell) on a group of one rank (torch.distributed's three calls answered in
    place, so no process group is needed) equals Viterbi.viterbi(x, cell) on the gene model."""
    import torch.distributed as dist
    from hmm_layer_amd import MsaHMMLayer as L5
    from hmm_layer_amd import Viterbi
    from test_layer_gpu import gene_setup
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: 1)
    monkeypatch.setattr(dist, "get_rank", lambda group=None: 0)
    monkeypatch.setattr(dist, "all_gather", lambda outs, x, group=None: outs[0].copy_(x))
    cell, x, A, _, _ = gene_setup(3, 900, seed=6)
    want_path, want_score = Viterbi.viterbi(x, cell)
    E = L5._engine_inputs(x, cell, None, False)[2]
    path, score = Viterbi.viterbi_sharded(E, cell)
    assert path.dtype == torch.int32 and tuple(path.shape) == (1, 3, 900)
    assert torch.equal(path, want_path) and torch.equal(score, want_score)
    p = path[0].cpu().numpy()
    assert bool((A[p[:, :-1], p[:, 1:]] > 0).all())         # every step of the path is an edge of the model


# ---- G: graph capture -----------------------------------------------------------------------------------------------
def test_g_three_calls_captured_into_one_graph():
    """reduce -> apply -> path of one rank on one stream, captured once and replayed: no host synchronisation, no
    helper stream; bit-identical to the eager calls."""
    logA, logpi, logE = (dev(x) for x in inputs("g15", "random", 3, sc.B_L))
    eager_path, eager_score = engine.viterbi(logA, logpi, logE)

    def three_calls():
        vop, vbase = engine.seqshard_viterbi_reduce(logA, logpi, logE, True, 1)
        origin, final_state, score = engine.seqshard_viterbi_apply(logA, logpi, logE, vop.unsqueeze(2), vbase.unsqueeze(2), 0)
        return engine.seqshard_viterbi_path(tuple(logE.shape), origin.unsqueeze(2), final_state, 0), score

    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):          # one stream, no branches
            path, score = three_calls()
    path.fill_(-1)                                             # capture does not run the kernels; replay does
    score.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(path, eager_path) and torch.equal(score, eager_score)
