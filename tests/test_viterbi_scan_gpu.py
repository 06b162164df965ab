"""hmm_viterbi_scan (engine.viterbi_scan, the time-parallel chunk scan for up to 64 states) against the serial
definition (tests/viterbi_wide.py, oracle/viterbi.py) and against hmm_viterbi itself: paths and scores BIT-EXACT,
under forced and default chunk lengths, one- and two-level chunk scans, the sparse and the all-candidates reduce."""
import numpy as np
import pytest
import torch

from hmm_layer_amd import engine
from oracle import params
from oracle import viterbi as ov
from tests import viterbi_wide as vw

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SCAN2_MIN_C = 32            # chunks per sequence from which both chunk scans run in two levels (hmm_engine.hip)


def dev(x):
    return torch.as_tensor(np.asarray(x), dtype=torch.float32, device=DEV)


def scan(logA, logpi, logE, chunk=0, fn=None):
    """logA (k,q,q), logpi (k,q), logE (k,b,L,q) numpy or tensors -> (path, score) numpy under OPT_CHUNK = chunk."""
    fn = fn or engine.viterbi_scan
    with engine.option(engine.OPT_CHUNK, chunk):
        path, score = fn(dev(logA), dev(logpi), dev(logE))
        torch.cuda.synchronize()
    return path.cpu().numpy(), score.cpu().numpy()


def walk_t(logA, logpi, logE):
    """lib().hmm_viterbi directly (device tensors in and out): the one-wave-per-sequence walk for 17..64 states,
    the 16-state scan below — whatever engine.viterbi routes to."""
    lib = engine.lib()
    k, b, L, q = logE.shape
    need = lib.hmm_viterbi_workspace_bytes(k, b, L, q)
    ws = torch.empty(max(need, 256), dtype=torch.uint8, device=DEV)
    path = torch.empty((k, b, L), dtype=torch.int32, device=DEV)
    score = torch.empty((k, b), dtype=torch.float64, device=DEV)
    rc = lib.hmm_viterbi(logA.data_ptr(), logpi.data_ptr(), logE.data_ptr(), k, b, L, q, path.data_ptr(),
                         score.data_ptr(), ws.data_ptr(), ws.numel(), engine._stream(logE.device))
    assert rc == 0
    torch.cuda.synchronize()
    return path, score


def walk(logA, logpi, logE):
    path, score = walk_t(dev(logA).contiguous(), dev(logpi).contiguous(), dev(logE).contiguous())
    return path.cpu().numpy(), score.cpu().numpy()


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def gene_k_logs(k):
    from hmm_layer_amd.gene_pred_hmm_transitioner import GenePredMultiHMMTransitioner
    tr = GenePredMultiHMMTransitioner(k=k, initial_exon_len=200, initial_intron_len=4500, initial_ir_len=10000)
    with torch.no_grad():
        A = tr.make_A()[0].numpy().copy()
        pi = tr.make_initial_distribution().reshape(-1).numpy().copy()
    with np.errstate(divide="ignore"):
        return np.log(A).astype(np.float32), np.log(pi).astype(np.float32)


# ---------------------------------------------------------------- 1. shapes against the oracle
QS = (1, 2, 16, 17, 29, 31, 32, 33, 43, 48, 63, 64)
LS_CHUNK16 = (1, 2, 15, 16, 17, 31, 32, 33, 300)     # one position, a short chunk, exactly one, one plus one, a ragged tail
LS_DEFAULT = (1, 700, 3001)


@pytest.mark.parametrize("kind", ["dense", "sparse", "band"])
@pytest.mark.parametrize("q", QS)
def test_bit_exact_against_the_oracle(q, kind):
    rng = np.random.default_rng(1000 * q + len(kind))
    logA, logpi = vw.random_model(rng, q, kind)
    for chunk, lengths in ((16, LS_CHUNK16), (0, LS_DEFAULT)):
        for L in lengths:
            logE = vw.random_logE(rng, 5, L, q)
            wp, ws = vw.viterbi(logA, logpi, logE)           # once per (model, L); b = 1, 3 are its first rows
            for b in (1, 3, 5):
                gp, gs = scan(logA[None], logpi[None], logE[None, :b], chunk)
                tag = (q, kind, chunk, L, b)
                assert np.array_equal(gs[0], ws[:b]), (tag, gs[0], ws[:b])
                bad = np.argwhere(gp[0] != wp[:b])
                assert len(bad) == 0, (tag, len(bad), bad[:5].tolist())


# ---------------------------------------------------------------- 2. equals hmm_viterbi
def test_equals_hmm_viterbi():
    rng = np.random.default_rng(11)
    with np.errstate(divide="ignore"):
        g15 = np.log(params.intended_A15().numpy()).astype(np.float32), np.full(15, np.log(1 / 15), np.float32)
    models = [vw.random_model(rng, 3, "dense"), g15, gene_k_logs(2), gene_k_logs(3), vw.random_model(rng, 64, "band"),
              vw.random_model(rng, 43, "sparse"), gene_k_logs(4)]
    assert [m[0].shape[0] for m in models] == [3, 15, 29, 43, 64, 43, 57]
    for logA, logpi in models:
        q = logA.shape[0]
        logE = vw.random_logE(rng, 5, 300, q, dead=0.2)
        got = scan(logA[None], logpi[None], logE[None])
        want = walk(logA[None], logpi[None], logE[None])
        assert same(got, want), q
        wp, ws = vw.viterbi(logA, logpi, logE)
        assert np.array_equal(got[0][0], wp) and np.array_equal(got[1][0], ws), q


# ---------------------------------------------------------------- 3. ties and the clamp
@pytest.mark.parametrize("q", [29, 64])
def test_ties_take_the_lowest_index(q):
    """A uniform matrix and emissions drawn from three values (ties everywhere); inputs at the -1024 clamp almost
    everywhere (the off-edge candidate against explicit edges at the floor)."""
    rng = np.random.default_rng(q + 1)
    logA = np.full((q, q), np.log(1.0 / q), dtype=np.float32)
    logpi = np.full(q, np.log(1.0 / q), dtype=np.float32)
    logE = np.log(np.array([0.25, 0.5, 1.0], dtype=np.float32))[rng.integers(0, 3, (9, 300, q))]
    cA, cpi = vw.random_model(rng, q, "sparse")
    cA = np.where(rng.random(cA.shape) < 0.97, -np.inf, cA).astype(np.float32)
    cE = np.full((5, 300, q), -2000.0, dtype=np.float32)
    cE[rng.random(cE.shape) < 0.02] = -1.0
    cpi[:] = -np.inf
    for A, pi, E, tag in ((logA, logpi, logE, "uniform"), (cA, cpi, cE, "clamp")):
        wp, ws = vw.viterbi(A, pi, E)
        for chunk in (16, 0):
            got = scan(A[None], pi[None], E[None], chunk)
            assert np.array_equal(got[1][0], ws), (tag, chunk)
            assert np.array_equal(got[0][0], wp), (tag, chunk, np.argwhere(got[0][0] != wp)[:5].tolist())
            # the sparse reduce against the all-candidates reduce on the same input
            with engine.option(engine.OPT_FORCE_DENSE, 1):
                dense = scan(A[None], pi[None], E[None], chunk)
            assert same(got, dense), (tag, chunk)


# ---------------------------------------------------------------- 4. two-level chunk scans
@pytest.mark.parametrize("L", [16 * 40, 16 * 6 * 7 + 1, 16 * 9 * 9 + 1])
def test_two_level_scans_match_single_level_and_the_oracle(L):
    """One sequence, q = 43 sparse, chunks of 16: from SCAN2_MIN_C = 32 chunks on (L >= 16 * 31 + 1 = 497) both chunk
    scans run over groups of ceil(sqrt(C)) chunks.  L = 640: 40 chunks, 6 groups of 7 (the last one short);
    673 = 16 * 42 + 1: 43 chunks in groups of 7, one position into a new group; 1297 = 16 * 81 + 1: 82 chunks in groups
    of 10, likewise one more than a multiple of the previous group size 9."""
    q = 43
    assert L >= 16 * (SCAN2_MIN_C - 1) + 1
    rng = np.random.default_rng(L)
    logA, logpi = vw.random_model(rng, q, "sparse")
    logE = vw.random_logE(rng, 1, L, q)
    wp, ws = vw.viterbi(logA, logpi, logE)
    res = []
    for two in (0, 1):
        with engine.option(engine.OPT_SCAN2, two):
            res.append(scan(logA[None], logpi[None], logE[None], 16))
    assert same(res[0], res[1])
    assert np.array_equal(res[1][0][0], wp) and np.array_equal(res[1][1][0], ws)


# ---------------------------------------------------------------- 5. several models in one call
@pytest.mark.parametrize("copies", [2, 3])
def test_three_models_in_one_call(copies):
    """A sparse gene model, a dense model and a model with a state that no edge enters, all of 29 (43) states."""
    rng = np.random.default_rng(copies)
    g = gene_k_logs(copies)
    q = g[0].shape[0]
    dn = vw.random_model(rng, q, "dense")
    sp = vw.random_model(rng, q, "sparse")
    sp[0][:, 5] = -np.inf                                     # nothing enters state 5
    models = [g, dn, sp]
    logE = np.stack([vw.random_logE(rng, 3, 500, q) for _ in models])
    got = scan(np.stack([m[0] for m in models]), np.stack([m[1] for m in models]), logE)
    for m, (logA, logpi) in enumerate(models):
        wp, ws = vw.viterbi(logA, logpi, logE[m])
        assert np.array_equal(got[0][m], wp) and np.array_equal(got[1][m], ws), m


# ---------------------------------------------------------------- 6. long sequences
@pytest.mark.parametrize("b,L", [(1, 40000), (2, 20001)])
def test_long_sequences_equal_the_walk(b, L):
    logA, logpi = gene_k_logs(3)
    q = logA.shape[0]
    g = torch.Generator(device=DEV).manual_seed(L)
    logE = -6 * torch.rand((1, b, L, q), generator=g, device=DEV)
    A, pi = dev(logA)[None].contiguous(), dev(logpi)[None].contiguous()
    path, score = engine.viterbi_scan(A, pi, logE)
    wpath, wscore = walk_t(A, pi, logE)
    assert torch.equal(path, wpath) and torch.equal(score, wscore)
    Eh = logE[0].cpu().numpy()
    for r in range(b):
        assert ov.path_score(logA, logpi, Eh[r], path[0, r].cpu().numpy()) == float(score[0, r])


# ---------------------------------------------------------------- 7. offsets beyond 2^31
def test_offsets_beyond_2_to_31():
    k, b, L, q = 1, 2, 17000000, 17
    assert b * L * 64 > 2 ** 31 and b * L * q * 4 > 2 ** 31      # backpointer bytes, bytes of logE
    rng = np.random.default_rng(17)
    logA, logpi = vw.random_model(rng, q, "sparse")
    g = torch.Generator(device=DEV).manual_seed(7)
    logE = torch.rand((k, b, L, q), generator=g, device=DEV).mul_(-6)
    A, pi = dev(logA)[None].contiguous(), dev(logpi)[None].contiguous()
    path, score = engine.viterbi_scan(A, pi, logE)
    torch.cuda.synchronize()
    engine.release_workspaces()
    wpath, wscore = walk_t(A, pi, logE)
    for r in range(b):
        assert torch.equal(path[0, r], wpath[0, r]) and torch.equal(score[0, r], wscore[0, r]), r


# ---------------------------------------------------------------- 8. determinism, graph capture
def test_deterministic_and_capturable():
    rng = np.random.default_rng(8)
    logA, logpi = gene_k_logs(2)
    q = logA.shape[0]
    A, pi = dev(logA)[None].contiguous(), dev(logpi)[None].contiguous()
    logE = dev(vw.random_logE(rng, 3, 2500, q)[None]).contiguous()
    p1, s1 = engine.viterbi_scan(A, pi, logE)
    p2, s2 = engine.viterbi_scan(A, pi, logE)
    torch.cuda.synchronize()
    assert torch.equal(p1, p2) and torch.equal(s1, s2)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        engine.viterbi_scan(A, pi, logE)                      # warm-up on s: workspace allocated outside the capture
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            pg, sg = engine.viterbi_scan(A, pi, logE)
    E2 = dev(vw.random_logE(rng, 3, 2500, q)[None]).contiguous()
    want = engine.viterbi_scan(A, pi, E2)
    torch.cuda.synchronize()
    logE.copy_(E2)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(pg, want[0]) and torch.equal(sg, want[1])
    wp, ws = vw.viterbi(logA, logpi, E2[0].cpu().numpy())
    assert np.array_equal(pg[0].cpu().numpy(), wp) and np.array_equal(sg[0].cpu().numpy(), ws)


# ---------------------------------------------------------------- 9. routing
def routed_shapes():
    """One shape that hmm_viterbi_scan_pays sends to the scan (if the measured rule has any) and one it does not."""
    lib = engine.lib()
    shapes = [(1, 1, 6000, 29), (1, 1, 20000, 29), (1, 2, 100000, 29), (1, 1, 200000, 29)]
    yes = [s for s in shapes if lib.hmm_viterbi_scan_pays(*s)][:1]
    no = [(1, 70, 40, 29)]
    assert not lib.hmm_viterbi_scan_pays(*no[0])
    return yes + no


def test_engine_viterbi_routes_by_the_measured_rule():
    logA, logpi = gene_k_logs(2)
    for k, b, L, q in routed_shapes():
        g = torch.Generator(device=DEV).manual_seed(L)
        logE = -6 * torch.rand((k, b, L, q), generator=g, device=DEV)
        A, pi = dev(logA)[None].contiguous(), dev(logpi)[None].contiguous()
        a = engine.viterbi(A, pi, logE)
        s = engine.viterbi_scan(A, pi, logE)
        torch.cuda.synchronize()
        assert torch.equal(a[0], s[0]) and torch.equal(a[1], s[1]), (k, b, L, q)
        rows = [0, b - 1]
        wp, ws = vw.viterbi(logA, logpi, logE[0, rows].cpu().numpy())
        assert np.array_equal(a[0][0, rows].cpu().numpy(), wp) and np.array_equal(a[1][0, rows].cpu().numpy(), ws)


def test_layer_viterbi_on_the_two_copy_gene_model():
    from hmm_layer_amd import Viterbi
    from hmm_layer_amd import MsaHMMLayer as L5
    from hmm_layer_amd.MsaHmmCell import HmmCell
    from hmm_layer_amd.gene_pred_hmm_emitter import GenePredHMMEmitter
    from hmm_layer_amd.gene_pred_hmm_transitioner import GenePredMultiHMMTransitioner
    codons = dict(start_codons=[("ATG", 1.)], stop_codons=[("TAG", .34), ("TAA", .33), ("TGA", .33)],
                  intron_begin_pattern=[("NGT", .99), ("NGC", .005), ("NAT", .005)],
                  intron_end_pattern=[("AGN", .99), ("ACN", .01)])
    b, L = 1, 5000
    g = torch.Generator().manual_seed(22)
    cls = torch.softmax(2 * torch.randn((1, b, L, 15), generator=g), -1)
    nuc = torch.nn.functional.one_hot(torch.randint(0, 5, (1, b, L), generator=g), 5).float()
    x = torch.cat([cls, nuc], -1).to(DEV)
    em = GenePredHMMEmitter(**codons, num_copies=2)
    em.build((1, b, L, 15))
    tr = GenePredMultiHMMTransitioner(k=2, initial_exon_len=200, initial_intron_len=4500, initial_ir_len=10000)
    cell = HmmCell([29], 15, em, tr).to(DEV)
    path, score = Viterbi.viterbi(x, cell)
    torch.cuda.synchronize()
    assert path.shape == (1, b, L) and path.dtype == torch.int32 and score.shape == (1, b)
    At, pit, Et = L5._engine_inputs(x, cell, None, False)
    logE = torch.log(torch.clamp_min(Et, cell.epsilon))[0].cpu().numpy()
    logA = torch.log(At)[0].cpu().numpy()
    logpi = torch.log(torch.clamp_min(pit, cell.epsilon))[0].cpu().numpy()
    wp, ws = vw.viterbi(logA, logpi, logE)
    assert np.array_equal(path[0].cpu().numpy(), wp) and np.array_equal(score[0].cpu().numpy(), ws)
