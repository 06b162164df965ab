"""Sequence-sharded Viterbi for up to 64 states on the engine (hmm_seqshard_vscan_reduce / _apply / _path): ranks played
one after another on one GPU, one stream (hence one workspace) per rank; all reduces first, then all applies, then all
paths, so the workspaces have to survive.  Everything is compared with array_equal: against engine.viterbi and
engine.viterbi_scan on the uncut tensor, against oracle/viterbi.py, and piece by piece against the int64 restatement
(tests/seqshard_vscan_ref.py); for 1 and 16 states also against the 16-state family (hmm_seqshard_viterbi_*).

"g29" / "g43" are the two- and three-copy gene models (sparse reduce); they keep their topology whatever the input kind:
"ties", "flat" and "absent" redraw the PRESENT edges only.  "dQ" is a dense model of Q states."""
import contextlib
import functools

import numpy as np
import pytest
import torch

import seqshard_cases as sc
import seqshard_vscan_ref as svr
from hmm_layer_amd import build as hbuild
from hmm_layer_amd import engine, seqshard, seqshard_vscan

pytestmark = pytest.mark.gpu

KINDS = svr.KINDS + ("einf", "ebig")
DENSE_QS = (17, 32, 33, 48, 64, 1, 16)
MODELS = ("g29", "g43") + tuple("d%d" % q for q in DENSE_QS)
B_MODELS = MODELS + ("g29+d29",)                             # a sparse and a dense model in one call
LONG_L, LONG_CUTS, LONG_MODELS = 1513, (0, 513, 1513), ("g29", "d64")


@pytest.fixture(scope="module", autouse=True)
def _built():
    hbuild.build()


def dev(x):
    return torch.as_tensor(np.array(x) if isinstance(x, np.ndarray) else x, device="cuda:0")     # (inputs are read-only)


def gene_k_logs(k):
    """tests/test_viterbi_scan_gpu.py::gene_k_logs."""
    from hmm_layer_amd.gene_pred_hmm_transitioner import GenePredMultiHMMTransitioner
    tr = GenePredMultiHMMTransitioner(k=k, initial_exon_len=200, initial_intron_len=4500, initial_ir_len=10000)
    with torch.no_grad():
        A = tr.make_A()[0].numpy().copy()
        pi = tr.make_initial_distribution().reshape(-1).numpy().copy()
    with np.errstate(divide="ignore"):
        return np.log(A).astype(np.float32), np.log(pi).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _single(name):
    q = int(name[1:])
    if name[0] == "g":
        logA, logpi = gene_k_logs((q - 1) // 14)
        assert logA.shape == (q, q)
        return logA, logpi
    rng = np.random.default_rng([53, q])
    A = rng.random((q, q)) ** 3 + 1e-3
    A /= A.sum(-1, keepdims=True)
    pi = rng.random(q) + 0.1
    return np.log(A).astype(np.float32), np.log(pi / pi.sum()).astype(np.float32)


@functools.lru_cache(maxsize=None)
def inputs(name, kind, b, L):
    """-> logA (k,q,q), logpi (k,q), logE (k,b,L,q) float32, read-only."""
    Ms = [_single(n) for n in name.split("+")]
    logA, logpi = np.stack([m[0] for m in Ms]), np.stack([m[1] for m in Ms])
    k, q = logA.shape[:2]
    rng = np.random.default_rng([43, B_MODELS.index(name), KINDS.index(kind), b, L])
    logE = np.log(rng.random((k, b, L, q)) * 0.9 + 0.05).astype(np.float32)
    present = np.isfinite(logA)
    if kind == "ties":
        logA = np.where(present, -rng.integers(0, 3, logA.shape), -np.inf).astype(np.float32)
        logpi = -rng.integers(0, 3, logpi.shape).astype(np.float32)
        logE = -rng.integers(0, 3, logE.shape).astype(np.float32)
    elif kind == "flat":
        logA = np.where(present, -1.5, -np.inf).astype(np.float32)
        logpi, logE = np.full_like(logpi, -1.5), np.full_like(logE, -1.5)
    elif kind == "absent":
        logA = np.where(present & (rng.random(logA.shape) >= 0.6), logA, -np.inf).astype(np.float32)
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
    """engine.viterbi (the walk above 16 states) and engine.viterbi_scan on the uncut tensor: they have to agree."""
    path, score = engine.viterbi(dev(logA), dev(logpi), dev(logE))
    spath, sscore = engine.viterbi_scan(dev(logA), dev(logpi), dev(logE))
    assert torch.equal(path, spath) and torch.equal(score, sscore)
    return path.cpu().numpy(), score.cpu().numpy()


@functools.lru_cache(maxsize=None)
def rank_stream(r):
    return torch.cuda.Stream()                               # (kept: the engine caches one workspace per stream)


def engine_cuts(logA, logpi, logE, cuts, backend=seqshard_vscan.VscanEngineBackend):
    streams = [rank_stream(r) for r in range(len(cuts) - 1)]
    return svr.run_cuts(lambda r: (backend(), torch.cuda.stream(streams[r])), logA, logpi, logE, cuts, dev=dev,
                        sync=torch.cuda.synchronize)


def check_against(got, want_path, want_score, what):
    assert got["path"].dtype == np.int32
    assert np.array_equal(got["path"], want_path), what
    for r, s in enumerate(got["scores"]):
        assert np.array_equal(s, want_score), "%s: score on rank %d" % (what, r)


def full(vop, vbase, q):
    return vop.astype(np.int64)[..., :q, :q] + vbase[..., None, :q]


# ---- A: the slab operator alone -------------------------------------------------------------------------------------
A_MODELS = [(m, 0) for m in MODELS] + [("g29", 1), ("g43", 1)]
A_LENGTHS = {0: (1, 2, 15, 16, 17, 33, 100), 16: (496, 512, 513, 1000)}    # chunk 16: 31 / 32 / 33 / 63 chunks


@functools.lru_cache(maxsize=None)
def a_reference(name, chunk, seq_start):
    """The restatement's operators of the slabs logE[:, :, :Ls], Ls in A_LENGTHS[chunk], from one pass."""
    logA, logpi, logE = inputs(name, "random", 3, max(A_LENGTHS[chunk]))
    return [(v.numpy(), w.numpy()) for v, w in svr.slab_operators(logA, logpi, logE, seq_start, A_LENGTHS[chunk])]


@pytest.mark.parametrize("chunk", sorted(A_LENGTHS))
@pytest.mark.parametrize("name,force_dense", A_MODELS)
def test_a_slab_operator(name, force_dense, chunk):
    logA, logpi, logE = inputs(name, "random", 3, max(A_LENGTHS[chunk]))
    q = logE.shape[-1]
    QT = svr.tile(q)
    with engine.option(engine.OPT_CHUNK, chunk), engine.option(engine.OPT_FORCE_DENSE, force_dense):
        for seq_start in (0, 1):
            want = a_reference(name, chunk, seq_start)
            for Ls, (wop, wbase) in zip(A_LENGTHS[chunk], want):
                vop, vbase = seqshard_vscan.reduce(dev(logA), dev(logpi), dev(logE[:, :, :Ls]), seq_start, 2)
                vop, vbase = vop.cpu().numpy(), vbase.cpu().numpy()
                what = "%s Ls=%d seq_start=%d" % (name, Ls, seq_start)
                assert vop.shape == (1, 3, QT, QT) and vbase.shape == (1, 3, QT), what
                assert np.array_equal(full(vop, vbase, q), full(wop, wbase, q)), what
                assert not vop[..., :q, :q].max(-2).any(), what                # every column has maximum 0
                assert np.array_equal(vop, wop) and np.array_equal(vbase, wbase), what     # the padding, as the header states it
                if seq_start:
                    assert np.array_equal(full(vop, vbase, q), np.broadcast_to(full(vop, vbase, q)[..., :1], (1, 3, q, q))), what


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
        if q <= 16:                                          # where both families run they agree
            small = engine_cuts(logA, logpi, logE, cuts, backend=seqshard.ViterbiEngineBackend)
            check_against(small, got["path"], got["scores"][0], "the 16-state family, cuts %s" % (cuts,))
            for r in range(len(cuts) - 1):
                assert np.array_equal(full(small["vops"][r], small["vbases"][r], q), full(got["vops"][r], got["vbases"][r], q))
                assert np.array_equal(small["origins"][r][..., :q], got["origins"][r][..., :q])
        if cuts == B_REF_CUT:
            ref = svr.run_cuts(lambda r: (svr.RefVscanBackend(), contextlib.nullcontext()), logA, logpi, logE, cuts)
            for r in range(len(cuts) - 1):
                assert np.array_equal(full(got["vops"][r], got["vbases"][r], q), full(ref["vops"][r], ref["vbases"][r], q)), \
                    "operator of rank %d" % r
                assert np.array_equal(got["origins"][r], ref["origins"][r]), "map of rank %d" % r
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
        assert (np.abs(got["vbases"][r][..., :logE.shape[-1]]) > (1 << 31)).all()


# ---- E: R = 1, and the three calls repeated -------------------------------------------------------------------------
@pytest.mark.parametrize("name,L,chunk", [("g29", sc.B_L, 0), ("d33", sc.B_L, 0), ("g29+d29", LONG_L, 16), ("d64", 1, 0)])
def test_e_single_rank_equals_the_unsharded_call(name, L, chunk):
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
def test_f_viterbi_sharded_on_a_29_state_cell(monkeypatch):
    """Viterbi.viterbi_sharded(E_slab, cell) on a group of one rank (torch.distributed's three calls answered in
    place, so no process group is needed) equals Viterbi.viterbi(x, cell) on the two-copy gene model: seqshard.viterbi
    picks the 64-state backend from q."""
    import torch.distributed as dist
    from hmm_layer_amd import MsaHMMLayer as L5
    from hmm_layer_amd import Viterbi
    from hmm_layer_amd.MsaHmmCell import HmmCell
    from hmm_layer_amd.gene_pred_hmm_emitter import GenePredHMMEmitter
    from hmm_layer_amd.gene_pred_hmm_transitioner import GenePredMultiHMMTransitioner
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: 1)
    monkeypatch.setattr(dist, "get_rank", lambda group=None: 0)
    monkeypatch.setattr(dist, "all_gather", lambda outs, x, group=None: outs[0].copy_(x))
    codons = dict(start_codons=[("ATG", 1.)], stop_codons=[("TAG", .34), ("TAA", .33), ("TGA", .33)],
                  intron_begin_pattern=[("NGT", .99), ("NGC", .005), ("NAT", .005)],
                  intron_end_pattern=[("AGN", .99), ("ACN", .01)])
    b, L = 3, 900
    g = torch.Generator().manual_seed(23)
    cls = torch.softmax(2 * torch.randn((1, b, L, 15), generator=g), -1)
    nuc = torch.nn.functional.one_hot(torch.randint(0, 5, (1, b, L), generator=g), 5).float()
    x = torch.cat([cls, nuc], -1).to("cuda:0")
    em = GenePredHMMEmitter(**codons, num_copies=2)
    em.build((1, b, L, 15))
    tr = GenePredMultiHMMTransitioner(k=2, initial_exon_len=200, initial_intron_len=4500, initial_ir_len=10000)
    cell = HmmCell([29], 15, em, tr).to("cuda:0")
    want_path, want_score = Viterbi.viterbi(x, cell)
    E = L5._engine_inputs(x, cell, None, False)[2]
    assert E.shape[-1] == 29
    path, score = Viterbi.viterbi_sharded(E, cell)
    assert path.dtype == torch.int32 and tuple(path.shape) == (1, b, L)
    assert torch.equal(path, want_path) and torch.equal(score, want_score)
    with pytest.raises(ValueError, match="64"):
        seqshard.viterbi(torch.zeros(1, 65, 65), torch.zeros(1, 65), torch.zeros(1, 1, 4, 65))


# ---- G: graph capture -----------------------------------------------------------------------------------------------
def test_g_three_calls_captured_into_one_graph():
    """reduce -> apply -> path of one rank on one stream, captured once and replayed: no host synchronisation, no
    helper stream; bit-identical to the eager calls."""
    logA, logpi, logE = (dev(x) for x in inputs("g29", "random", 3, sc.B_L))
    eager_path, eager_score = engine.viterbi(logA, logpi, logE)

    def three_calls():
        vop, vbase = seqshard_vscan.reduce(logA, logpi, logE, True, 1)
        origin, final_state, score = seqshard_vscan.apply(logA, logpi, logE, vop.unsqueeze(2), vbase.unsqueeze(2), 0)
        return seqshard_vscan.path(tuple(logE.shape), origin.unsqueeze(2), final_state, 0), score

    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        three_calls()                                          # warm-up: the workspace is allocated outside the capture
    stream.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):          # one stream, no branches
            path, score = three_calls()
    path.fill_(-1)                                             # capture does not run the kernels; replay does
    score.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(path, eager_path) and torch.equal(score, eager_score)
