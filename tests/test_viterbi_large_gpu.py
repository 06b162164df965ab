"""hmm_viterbi_large (engine.viterbi_large, q up to 4096) against the wide restatement (tests/viterbi_wide.py):
paths and scores BIT-EXACT, under both evaluations (HMM_OPT_VLARGE = 1 per-sequence walk, 2 per-position tiles)."""
import numpy as np
import pytest
import torch

from hmm_layer_amd import engine
from oracle import params
from oracle import viterbi as ov
from tests import viterbi_wide as vw

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WALK_MAX = 1024


def dev(x):
    return torch.as_tensor(np.asarray(x), dtype=torch.float32, device=DEV)


def run(logA, logpi, logE, route=0, fn=None):
    """logA (k,q,q), logpi (k,q), logE (k,b,L,q) numpy -> (path, score) numpy under OPT_VLARGE = route."""
    fn = fn or engine.viterbi_large
    with engine.option(engine.OPT_VLARGE, route):
        path, score = fn(dev(logA), dev(logpi), dev(logE))
        torch.cuda.synchronize()
    return path.cpu().numpy(), score.cpu().numpy()


def sample_rows(b):
    return sorted({r for r in (0, 1, 63, 64, 65, b // 2, b - 1) if 0 <= r < b})


def check_both(logA, logpi, logE, tag, rows=None):
    """Both evaluations (the walk only where q <= 1024) equal each other and, on `rows` (default: all), the
    restatement.  logA (k,q,q), logpi (k,q), logE (k,b,L,q)."""
    k, b, L, q = logE.shape
    routes = (1, 2) if q <= WALK_MAX else (2,)
    got = [run(logA, logpi, logE, r) for r in routes]
    for g in got[1:]:
        assert np.array_equal(g[0], got[0][0]) and np.array_equal(g[1], got[0][1]), tag
    rows = range(b) if rows is None else rows
    for m in range(k):
        rs = list(rows)
        wp, ws = vw.viterbi(logA[m], logpi[m], logE[m][rs])
        gp, gs = got[0][0][m][rs], got[0][1][m][rs]
        assert np.array_equal(gs, ws), (tag, m, gs[:3], ws[:3])
        bad = np.argwhere(gp != wp)
        assert len(bad) == 0, (tag, m, len(bad), bad[:5].tolist())
    return got[0]


CASES = [  # q, b, L, kind
    (65, 63, 37, "dense"), (71, 65, 37, "sparse"), (127, 1, 37, "band"), (128, 65, 2, "sparse"),
    (129, 63, 37, "band"), (255, 1, 37, "sparse"), (256, 65, 2, "dense"), (257, 63, 1, "band"),
    (344, 65, 37, "sparse"), (1027, 1, 37, "band"), (1027, 65, 2, "sparse"), (4096, 1, 2, "dense"),
    (4096, 2, 1, "sparse"), (1024, 3, 9, "sparse"), (1000, 2, 5, "dense"),
]


@pytest.mark.parametrize("q,b,L,kind", CASES)
def test_bit_exact_against_the_restatement(q, b, L, kind):
    rng = np.random.default_rng(q * 7 + b + L)
    logA, logpi = vw.random_model(rng, q, kind)
    logE = vw.random_logE(rng, b, L, q)
    rows = None if q * q * b * L < 3e8 else sample_rows(b)
    check_both(logA[None], logpi[None], logE[None], "q=%d b=%d L=%d %s" % (q, b, L, kind), rows)


@pytest.mark.parametrize("q", [71, 300])
def test_two_models_with_their_own_matrices(q):
    rng = np.random.default_rng(q)
    la0, lp0 = vw.random_model(rng, q, "sparse")
    la1, lp1 = vw.random_model(rng, q, "band")
    logE = np.stack([vw.random_logE(rng, 65, 11, q), vw.random_logE(rng, 65, 11, q)])
    check_both(np.stack([la0, la1]), np.stack([lp0, lp1]), logE, "k=2 q=%d" % q, rows=sample_rows(65))


@pytest.mark.parametrize("q", [100, 200])
def test_ties_take_the_lowest_index(q):
    """A uniform matrix and emissions drawn from three values (ties everywhere); inputs at the -1024 clamp
    almost everywhere (the off-edge candidate against explicit edges at the floor)."""
    rng = np.random.default_rng(q + 1)
    logA = np.full((q, q), np.log(1.0 / q), dtype=np.float32)
    logpi = np.full(q, np.log(1.0 / q), dtype=np.float32)
    logE = np.log(np.array([0.25, 0.5, 1.0], dtype=np.float32))[rng.integers(0, 3, (9, 13, q))]
    check_both(logA[None], logpi[None], logE[None], "uniform q=%d" % q)
    cA, cpi = vw.random_model(rng, q, "sparse")
    cA = np.where(rng.random(cA.shape) < 0.97, -np.inf, cA).astype(np.float32)
    cE = np.full((5, 17, q), -2000.0, dtype=np.float32)
    cE[rng.random(cE.shape) < 0.02] = -1.0
    cpi[:] = -np.inf
    check_both(cA[None], cpi[None], cE[None], "clamp q=%d" % q)
    # the sparse step forced dense on the same input
    got = run(cA[None], cpi[None], cE[None], 1)
    with engine.option(engine.OPT_FORCE_DENSE, 1):
        dense = run(cA[None], cpi[None], cE[None], 1)
    assert np.array_equal(got[0], dense[0]) and np.array_equal(got[1], dense[1])


def gene_k_logs(k):
    from hmm_layer_amd.gene_pred_hmm_transitioner import GenePredMultiHMMTransitioner
    tr = GenePredMultiHMMTransitioner(k=k, initial_exon_len=200, initial_intron_len=4500, initial_ir_len=10000)
    with torch.no_grad():
        A = tr.make_A()[0].numpy().copy()
        pi = tr.make_initial_distribution().reshape(-1).numpy().copy()
    with np.errstate(divide="ignore"):
        return np.log(A).astype(np.float32), np.log(pi).astype(np.float32)


def test_equals_hmm_viterbi_up_to_64_states():
    rng = np.random.default_rng(11)
    with np.errstate(divide="ignore"):
        g15 = np.log(params.intended_A15().numpy()).astype(np.float32), np.full(15, np.log(1 / 15), np.float32)
    models = [vw.random_model(rng, 3, "dense"), g15, gene_k_logs(2), gene_k_logs(3), vw.random_model(rng, 64, "band"),
              vw.random_model(rng, 43, "sparse")]
    for logA, logpi in models:
        q = logA.shape[0]
        logE = vw.random_logE(rng, 5, 300, q, dead=0.2)
        want = run(logA[None], logpi[None], logE[None], 0, fn=engine.viterbi)     # hmm_viterbi
        for route in (0, 1, 2):
            got = run(logA[None], logpi[None], logE[None], route)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (q, route)


def test_config5_shape():
    """BASELINE configs[4]: b = 1024 sequences of a 1027-state profile-like model, L = 6, on the tiles."""
    b, q, L = 1024, 1027, 6
    rng = np.random.default_rng(5)
    logA, logpi = vw.random_model(rng, q, "band")
    logE = vw.random_logE(rng, b, L, q, dead=0.02)
    path, score = run(logA[None], logpi[None], logE[None], 0)
    rows = sample_rows(b)
    wp, ws = vw.viterbi(logA, logpi, logE[rows])
    assert np.array_equal(path[0][rows], wp) and np.array_equal(score[0][rows], ws)
    for r in rows:
        assert ov.path_score(logA, logpi, logE[r], path[0][r]) == score[0][r]


def test_layer_viterbi_on_the_five_copy_gene_model():
    from hmm_layer_amd import Viterbi
    from hmm_layer_amd import MsaHMMLayer as L5
    from hmm_layer_amd.MsaHmmCell import HmmCell
    from hmm_layer_amd.gene_pred_hmm_emitter import GenePredHMMEmitter
    from hmm_layer_amd.gene_pred_hmm_transitioner import GenePredMultiHMMTransitioner
    codons = dict(start_codons=[("ATG", 1.)], stop_codons=[("TAG", .34), ("TAA", .33), ("TGA", .33)],
                  intron_begin_pattern=[("NGT", .99), ("NGC", .005), ("NAT", .005)],
                  intron_end_pattern=[("AGN", .99), ("ACN", .01)])
    b, L = 3, 400
    g = torch.Generator().manual_seed(21)
    cls = torch.softmax(2 * torch.randn((1, b, L, 15), generator=g), -1)
    nuc = torch.nn.functional.one_hot(torch.randint(0, 5, (1, b, L), generator=g), 5).float()
    x = torch.cat([cls, nuc], -1).to(DEV)
    em = GenePredHMMEmitter(**codons, num_copies=5)
    em.build((1, b, L, 15))
    tr = GenePredMultiHMMTransitioner(k=5, initial_exon_len=200, initial_intron_len=4500, initial_ir_len=10000)
    cell = HmmCell([71], 15, em, tr).to(DEV)
    path, score = Viterbi.viterbi(x, cell)
    torch.cuda.synchronize()
    assert path.shape == (1, b, L) and path.dtype == torch.int32 and score.shape == (1, b)
    At, pit, Et = L5._engine_inputs(x, cell, None, False)
    logE = torch.log(torch.clamp_min(Et, cell.epsilon))[0].cpu().numpy()
    logA = torch.log(At)[0].cpu().numpy()
    logpi = torch.log(torch.clamp_min(pit, cell.epsilon))[0].cpu().numpy()
    wp, ws = vw.viterbi(logA, logpi, logE)
    assert np.array_equal(path[0].cpu().numpy(), wp) and np.array_equal(score[0].cpu().numpy(), ws)
    p = path[0].cpu().numpy()
    A = At[0].cpu().numpy()
    assert bool((A[p[:, :-1], p[:, 1:]] > 0).all())


def test_offsets_beyond_2_to_31():
    """k*b*L*q > 2^31 (backpointers beyond 4 GB): sampled sequences, the last included, under both evaluations."""
    k, b, L, q = 1, 1024, 30000, 71
    assert k * b * L * q > 2 ** 31
    logA, logpi = gene_k_logs(5)
    g = torch.Generator(device=DEV).manual_seed(9)
    logE = -6 * torch.rand((k, b, L, q), generator=g, device=DEV)
    rows = [0, 517, b - 1]
    res = []
    for route in (1, 2):
        with engine.option(engine.OPT_VLARGE, route):
            path, score = engine.viterbi_large(dev(logA)[None], dev(logpi)[None], logE)
            torch.cuda.synchronize()
        res.append((path[0, rows].cpu().numpy(), score[0, rows].cpu().numpy()))
        del path, score
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
    wp, ws = vw.viterbi(logA, logpi, logE[0, rows].cpu().numpy())
    assert np.array_equal(res[0][0], wp) and np.array_equal(res[0][1], ws)


def test_deterministic():
    rng = np.random.default_rng(2)
    for q, route in ((90, 1), (600, 2)):
        logA, logpi = vw.random_model(rng, q, "band")
        logE = vw.random_logE(rng, 70, 9, q)
        a = run(logA[None], logpi[None], logE[None], route)
        b2 = run(logA[None], logpi[None], logE[None], route)
        assert np.array_equal(a[0], b2[0]) and np.array_equal(a[1], b2[1])


def test_errors_and_routing_through_viterbi():
    lib = engine.lib()
    assert lib.hmm_viterbi_large_workspace_bytes(1, 1024, 6, 1027) > 0
    with pytest.raises(ValueError):
        engine.viterbi_large(dev(np.zeros((1, 4097, 4097))), dev(np.zeros((1, 4097))),
                             dev(np.zeros((1, 1, 1, 4097))))
    # engine.viterbi serves q > 64 through hmm_viterbi_large
    rng = np.random.default_rng(4)
    logA, logpi = vw.random_model(rng, 65, "dense")
    logE = vw.random_logE(rng, 2, 5, 65)
    a = run(logA[None], logpi[None], logE[None], 0, fn=engine.viterbi)
    b2 = run(logA[None], logpi[None], logE[None], 0)
    assert np.array_equal(a[0], b2[0]) and np.array_equal(a[1], b2[1])
