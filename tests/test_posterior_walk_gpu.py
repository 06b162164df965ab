"""engine.posterior_walk / hmm_posterior_walk and hmm_posterior_decode_wide on the device: posteriors and fused posterior
decoding by a per-sequence walk for 65..256 states (hmm_wideq.inc), on the sparse step (with 0, 1 and 2 hubs), the
dense step with A in registers (up to 128 states) and the slow dense step above.

  1  the walk's three modes and loglik against the fp64 oracle with the numbers of tests/largeq_sweep.py
     (posterior_walk_cases.check_walk); the same inputs through engine.posterior (the GEMMs) meet the same limits
  2  models on the step rule (in 1's case list), and HMM_OPT_FORCE_DENSE against the default
  3  bit-identities: loglik over the modes and the decode call, k = 2 against k = 1, the identity-map decode against
     posterior_walk(POST_PROB) (label = lowest argmax, conf = max)
  4  class maps against fp64 class sums of the walk's own gamma (tol(n), MARGIN_CAP) and against the oracle
     (n STATE_TOL, ORACLE_CAP; the cases tests/test_posterior_walk_cpu.py certifies)
  5  determinism on a dirtied workspace; graph capture and replay of both calls, the class table changed afterwards
  6  the routing of engine.posterior_decode and of the five-copy layer"""
import ctypes

import numpy as np
import pytest
import torch

import memory_contract_table as mct
import posterior_decode_ref as ref
import posterior_walk_cases as cases
from hmm_layer_amd import engine
from hmm_layer_amd.MsaHMMLayer import MsaHmmLayer, _engine_inputs
from test_engine_gpu import DEV, dev

gpu = pytest.mark.gpu
T = cases.T
MODES = (("prob", engine.POST_PROB), ("log", engine.POST_LOG), ("lognoll", engine.POST_LOG_NO_LL))


def walk_outputs(fn, A, pi, E, eps):
    """The three modes of fn (engine.posterior_walk or engine.posterior) -> dict of numpy arrays (leading k axis)."""
    A, pi, E = dev(A), dev(pi), dev(E)
    out = {}
    for name, mode in MODES:
        o, ll = fn(A, pi, E, mode=mode, eps=eps)
        out[name], out["ll_" + name] = o.cpu().numpy(), ll.cpu().numpy()
    return out


def decode_wide(A, pi, E, table=None, C=None, eps=engine.EPS, want_conf=True, want_ll=True, ws=None):
    """hmm_posterior_decode_wide through the C ABI (whatever hmm_posterior_walk_pays says) -> (label, conf, loglik)
    as device tensors."""
    A, pi, E = (x if torch.is_tensor(x) else dev(x) for x in (A, pi, E))
    k, b, L, q = E.shape
    need = engine.lib().hmm_posterior_decode_wide_workspace_bytes(k, b, L, q)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV) if ws is None else ws
    label = torch.full((k, b, L), 255, dtype=torch.uint8, device=DEV)
    conf = torch.full((k, b, L), -1.0, dtype=torch.float32, device=DEV) if want_conf else None
    ll = torch.zeros((k, b), dtype=torch.float64, device=DEV) if want_ll else None
    tab = (ctypes.c_int * q)(*table) if table is not None else None
    rc = engine.lib().hmm_posterior_decode_wide(A.data_ptr(), pi.data_ptr(), E.data_ptr(), k, b, L, q, eps, tab,
                                                C if table is not None else q, label.data_ptr(),
                                                conf.data_ptr() if want_conf else None,
                                                ll.data_ptr() if want_ll else None, ws.data_ptr(), ws.numel(),
                                                torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return label, conf, ll


def assert_identity(gamma, ll, dec, tag):
    label, conf, lld = dec
    gamma = gamma.cpu().numpy()
    assert np.array_equal(label.cpu().numpy(), gamma.argmax(-1).astype(np.uint8)), tag    # numpy: the first maximum
    assert np.array_equal(conf.cpu().numpy(), gamma.max(-1)), tag
    assert torch.equal(lld, ll), tag


def assert_classes(gamma, dec, table, C, tag):
    """Against fp64 class sums of the walk's own fp32 gamma."""
    label, conf = dec[0].cpu().numpy(), dec[1].cpu().numpy()
    n = cases.largest_class(table, C)
    want, cref, margin = ref.decode(gamma.cpu().numpy(), table, C)
    err = float(np.abs(conf - cref).max())
    sure = margin > 2 * cases.tol(n)
    left = float((~sure).mean())
    print("%s: n = %d, |conf - ref| max %.3g (bound %.3g), positions within the margin %.5f"
          % (tag, n, err, cases.tol(n), left))
    assert err <= cases.tol(n), (tag, err)
    assert left <= cases.MARGIN_CAP, (tag, left)
    assert np.array_equal(label[sure], want[sure]), tag
    unused = sorted(set(range(C)) - set(table))                  # an empty class sums to zero: never the label
    assert label.max() < C and not np.isin(label, unused).any(), tag


# ---------------------------------------------------------------- 1, 2. against the fp64 oracle

@gpu
@pytest.mark.parametrize("case", cases.walk_cases(), ids=lambda c: c[0])
def test_walk_against_the_fp64_oracle(case):
    tag, kind, q, (k, b, L), zero, blank, eps = case
    A, pi, E, eps, oracles = cases.walk_inputs(case)
    got = walk_outputs(engine.posterior_walk, A, pi, E, eps)
    gemm = walk_outputs(engine.posterior, A, pi, E, eps)
    fails = []
    for m in range(k):
        for name, res in (("walk", got), ("gemm", gemm)):
            f, fig = cases.check_walk({n: v[m] for n, v in res.items()}, oracles[m], "%s %s model %d" % (tag, name, m))
            print("%s %s model %d: prob %.1e log %.1e / %.1e noll %.1e / %.1e rows %.1e ll %+.1e" % (
                tag, name, m, fig["prob"], fig["log"], fig["log_logspace"], fig["lognoll"], fig["lognoll_logspace"],
                fig["rowsum"], fig["ll"]))
            fails += f
        if k > 1:                                            # the models of a call do not interact: bitwise
            one = walk_outputs(engine.posterior_walk, A[m:m + 1], pi[m:m + 1], E[m:m + 1], eps)
            for n in got:
                if not np.array_equal(one[n][0], got[n][m], equal_nan=True):
                    fails.append("%s model %d: %s of the k = %d call differs from the k = 1 call" % (tag, m, n, k))
    assert not fails, "\n".join(fails[:12])


@gpu
@pytest.mark.parametrize("q", cases.GENE_STATES)
def test_forced_dense_step_against_the_default(q):
    case = next(c for c in cases.walk_cases() if c[1] == "gene" and c[2] == q)
    A, pi, E, eps, oracles = cases.walk_inputs(case)
    got = {}
    for force in (0, 1):
        with engine.option(engine.OPT_FORCE_DENSE, force):
            got[force] = walk_outputs(engine.posterior_walk, A, pi, E, eps)
        for m in range(E.shape[0]):
            f, fig = cases.check_walk({n: v[m] for n, v in got[force].items()}, oracles[m], "force %d model %d" % (force, m))
            assert not f, "\n".join(f[:12])
    # the two steps add in different orders: were the outputs bitwise equal, the option would not have reached the kernel
    assert not np.array_equal(got[0]["prob"], got[1]["prob"])


# ---------------------------------------------------------------- 3. bit-identities

@gpu
@pytest.mark.parametrize("q", cases.STATES)
def test_identity_map_decode_equals_the_walk_bit_for_bit(q):
    rng = np.random.default_rng(3000 + q)
    kinds = (("gene", 0), ("gene", 1)) if q in cases.GENE_STATES else (("dense", 0), ("deg1", 0))
    for kind, force in kinds:                                 # both steps at every state count
        for L in cases.LENGTHS:
            k, b = (2, 3) if L == T + 1 else (1, 5 if L <= 3 else 3)
            A, pi = cases.models(rng, kind, q, k)
            E = cases.emissions(rng, k, b, L, q)
            with engine.option(engine.OPT_FORCE_DENSE, force):
                gamma, ll = engine.posterior_walk(dev(A), dev(pi), dev(E), mode=engine.POST_PROB)
                dec = decode_wide(A, pi, E)
                assert_identity(gamma, ll, dec, (kind, force, q, L))
                for mode in (engine.POST_LOG, engine.POST_LOG_NO_LL):
                    assert torch.equal(engine.posterior_walk(dev(A), dev(pi), dev(E), mode=mode)[1], ll), (kind, q, L)
    nc = decode_wide(A, pi, E, want_conf=False, want_ll=False)                   # conf and loglik NULL
    assert nc[1] is None and nc[2] is None and torch.equal(nc[0], dec[0])


@gpu
@pytest.mark.parametrize("q", [65, 128, 129, 256])
def test_uniform_model_ties_go_to_the_lowest_index(q):
    """Uniform A, pi and E: every state has the same posterior, classes of equal size tie exactly."""
    A = np.full((1, q, q), 1 / q, dtype=np.float32)
    pi = np.full((1, q), 1 / q, dtype=np.float32)
    E = np.full((1, 3, 2 * T + 1, q), 0.25, dtype=np.float32)
    gamma, ll = engine.posterior_walk(dev(A), dev(pi), dev(E), mode=engine.POST_PROB)
    dec = decode_wide(A, pi, E)
    assert_identity(gamma, ll, dec, q)
    assert not dec[0].any()
    if q % 16 == 0:
        label, conf, _ = decode_wide(A, pi, E, [i % 16 for i in range(q)], 16)
        assert not label.any() and np.allclose(conf.cpu().numpy(), 1 / 16, rtol=1e-5)


@gpu
def test_offsets_beyond_2_to_31():
    """k*b*L*q > 2^31 elements (E, out and the parking region beyond 8 GB): sampled sequences, the last included, equal
    bit for bit what the same sequences give in a call of their own, for the walk and for the decode call."""
    k, b, L, q = 1, 1024, 30000, 71
    assert k * b * L * q > 2 ** 31
    A, pi = cases.models(np.random.default_rng(31), "gene", q, 1)
    A, pi = dev(A), dev(pi)
    g = torch.Generator(device=DEV).manual_seed(9)
    E = torch.rand((k, b, L, q), generator=g, device=DEV).pow_(4).mul_(0.9).add_(0.05)
    rows = [0, 517, b - 1]
    Es = E[:, rows].contiguous()
    table = cases.gene_classes(q)
    gamma, ll = engine.posterior_walk(A, pi, E, mode=engine.POST_PROB)
    want, wll = engine.posterior_walk(A, pi, Es, mode=engine.POST_PROB)
    assert torch.equal(gamma[:, rows], want) and torch.equal(ll[:, rows], wll)
    assert bool(torch.isfinite(gamma[0, -1]).all()) and bool(torch.isfinite(gamma[0, :, -1]).all())
    del gamma
    torch.cuda.empty_cache()
    label, conf, lld = decode_wide(A, pi, E, table, 6)
    wl, wc, _ = decode_wide(A, pi, Es, table, 6)
    assert torch.equal(label[:, rows], wl) and torch.equal(conf[:, rows], wc) and torch.equal(lld, ll)
    assert int(label.max()) < 6 and int(label[0, -1].max()) > 0
    del E, label, conf
    torch.cuda.empty_cache()


# ---------------------------------------------------------------- 4. class maps

@gpu
@pytest.mark.parametrize("case", cases.class_cases(), ids=lambda c: c[0])
def test_class_maps_against_fp64_sums_of_the_walks_gamma(case):
    tag, kind, q, table, C, seed = case
    for shape in cases.CLASS_SHAPES:
        A, pi, E = cases.class_inputs(case, shape)
        gamma, ll = engine.posterior_walk(dev(A), dev(pi), dev(E), mode=engine.POST_PROB)
        dec = decode_wide(A, pi, E, table, C)
        assert_classes(gamma, dec, table, C, (tag,) + shape)
        assert torch.equal(dec[2], ll)


@gpu
@pytest.mark.parametrize("case", cases.oracle_cases(), ids=lambda c: c[0])
def test_decode_against_the_fp64_oracle(case):
    tag, kind, q, table, C, seed = case
    n = 1 if table is None else cases.largest_class(table, C)
    for shape in cases.ORACLE_SHAPES:
        A, pi, E, g64, ll64 = cases.oracle_inputs(case, shape)
        label, conf, ll = (t.cpu().numpy() for t in decode_wide(A, pi, E, table, C))
        want, c64, margin = ref.decode(g64, table, C)
        err = float(np.abs(conf - c64).max())
        sure = margin > 2 * n * cases.STATE_TOL
        print("%s %s: |conf - conf64| max %.3g (bound %.3g), positions within the margin %.4f"
              % (tag, shape, err, n * cases.STATE_TOL, (~sure).mean()))
        assert err <= n * cases.STATE_TOL
        assert (~sure).mean() <= cases.ORACLE_CAP
        assert np.array_equal(label[sure], want[sure])
        assert np.all(np.abs(ll - ll64) <= 1e-6 * np.abs(ll64) + 2e-4)


# ---------------------------------------------------------------- 5. determinism and capture

def _capture_inputs(q):
    rng = np.random.default_rng(q)
    A, pi = cases.models(rng, "gene" if q in cases.GENE_STATES else "dense", q, 1)
    shape = (1, 4, 150, q)
    return dev(A), dev(pi), shape


@gpu
@pytest.mark.parametrize("q", [71, 100, 253])
def test_repeated_calls_are_bit_identical_on_a_dirtied_workspace(q):
    A, pi, shape = _capture_inputs(q)
    E = 0.05 + 0.9 * torch.rand(shape, device=DEV) ** 4
    table = cases.random_map(np.random.default_rng(q), q, 6)
    need = engine.lib().hmm_posterior_decode_wide_workspace_bytes(*shape)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    runs = []
    for fill in (0x00, 0xFF):                                                   # 0xFF: every float and double a NaN
        ws.fill_(fill)
        runs.append([t.clone() for t in decode_wide(A, pi, E, table, 6, ws=ws)])
    for x, y in zip(*runs):
        assert torch.equal(x, y)
    wsw = engine._workspace(torch.device(DEV), 0, engine.WALK_TAG)
    first = [t.clone() for t in engine.posterior_walk(A, pi, E)]
    torch.cuda.synchronize()
    wsw.fill_(0xFF)
    second = engine.posterior_walk(A, pi, E)
    torch.cuda.synchronize()
    assert engine._workspace(torch.device(DEV), 0, engine.WALK_TAG).data_ptr() == wsw.data_ptr()
    for x, y in zip(first, second):
        assert torch.equal(x, y)


@gpu
@pytest.mark.parametrize("q", [71, 128])
def test_graph_capture_of_both_calls_keeps_the_class_table(q):
    A, pi, shape = _capture_inputs(q)
    k, b, L, _ = shape
    E = 0.05 + 0.9 * torch.rand(shape, device=DEV) ** 4
    classes = cases.random_map(np.random.default_rng(q + 1), q, 6)
    table = (ctypes.c_int * q)(*classes)
    lib = engine.lib()
    ws = torch.empty(lib.hmm_posterior_decode_wide_workspace_bytes(*shape), dtype=torch.uint8, device=DEV)
    wsw = torch.empty(lib.hmm_posterior_walk_workspace_bytes(*shape), dtype=torch.uint8, device=DEV)
    label = torch.zeros((k, b, L), dtype=torch.uint8, device=DEV)
    conf = torch.zeros((k, b, L), dtype=torch.float32, device=DEV)
    ll, llw = (torch.zeros((k, b), dtype=torch.float64, device=DEV) for _ in range(2))
    out = torch.zeros(shape, dtype=torch.float32, device=DEV)

    def calls(stream):
        rc = lib.hmm_posterior_decode_wide(A.data_ptr(), pi.data_ptr(), E.data_ptr(), *shape, engine.EPS, table, 6,
                                           label.data_ptr(), conf.data_ptr(), ll.data_ptr(), ws.data_ptr(), ws.numel(),
                                           stream.cuda_stream)
        assert rc == 0
        rc = lib.hmm_posterior_walk(A.data_ptr(), pi.data_ptr(), E.data_ptr(), *shape, engine.EPS, engine.POST_LOG,
                                    out.data_ptr(), llw.data_ptr(), wsw.data_ptr(), wsw.numel(), stream.cuda_stream)
        assert rc == 0

    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        calls(s)                                                                # warm-up on the capture stream
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            calls(s)
    E2 = 0.05 + 0.9 * torch.rand(shape, device=DEV) ** 4
    E.copy_(E2)
    for i in range(q):                                                          # the caller's table changes after the capture
        table[i] = 0
    for t in (label, conf, ll, llw, out):
        t.zero_()
    g.replay()
    torch.cuda.synchronize()
    want = decode_wide(A, pi, E2, classes, 6)
    for x, y in zip((label, conf, ll), want):
        assert torch.equal(x, y)
    wout, wll = engine.posterior_walk(A, pi, E2, mode=engine.POST_LOG)
    assert torch.equal(out, wout) and torch.equal(llw, wll)
    assert int(label.max()) > 0


# ---------------------------------------------------------------- 6. routing of the wrapper and of the layer

@pytest.fixture
def fused_only(monkeypatch):
    """engine.posterior_decode must not compose: the posterior is out of reach while the fixture holds."""
    real = engine.posterior

    def refuse(*a, **kw):
        raise AssertionError("posterior_decode composed engine.posterior")
    monkeypatch.setattr(engine, "posterior", refuse)
    return real


@gpu
@pytest.mark.parametrize("q,sparse", [(71, False), (71, True), (253, True)])
def test_wrapper_takes_the_fused_path(q, sparse, fused_only):
    rng = np.random.default_rng(q)
    A, pi = cases.models(rng, "gene", q, 1)
    E = cases.emissions(rng, 1, 3, 130, q)
    table = cases.gene_classes(q)
    gamma, llw = engine.posterior_walk(dev(A), dev(pi), dev(E), mode=engine.POST_PROB)
    for tab, C in ((None, None), (table, 6)):
        dec = engine.posterior_decode(dev(A), dev(pi), dev(E), tab, C, sparse=sparse)
        torch.cuda.synchronize()
        if tab is None:
            assert_identity(gamma, llw, dec, q)
        else:
            assert_classes(gamma, dec, table, 6, "q=%d" % q)
    label, conf, _ = engine.posterior_decode(dev(A), dev(pi), dev(E), table, 6, want_conf=False, sparse=sparse)
    assert conf is None and torch.equal(label, dec[0])


@gpu
@pytest.mark.parametrize("q,classes,sparse", [(253, 6, False), (71, 20, True), (300, 6, True)])
def test_wrapper_composes_elsewhere(q, classes, sparse, monkeypatch):
    rng = np.random.default_rng(q + classes)
    A, pi = cases.models(rng, "dense", q, 1)
    E = cases.emissions(rng, 1, 3, 40, q)
    table = cases.random_map(rng, q, classes)
    calls = []
    real = engine.posterior
    monkeypatch.setattr(engine, "posterior", lambda *a, **kw: calls.append(1) or real(*a, **kw))
    label, conf, ll = engine.posterior_decode(dev(A), dev(pi), dev(E), table, classes, sparse=sparse)
    assert calls == [1]
    gamma, _ = real(dev(A), dev(pi), dev(E))
    want, cref, _ = ref.decode(gamma.cpu().numpy(), table, classes)
    assert np.abs(conf.cpu().numpy() - cref).max() <= cases.tol(cases.largest_class(table, classes))
    assert int(label.max()) < classes


@gpu
def test_layer_posterior_decode_five_copy_gene_model(fused_only):
    from hmm_layer_amd.MsaHmmCell import HmmCell
    from hmm_layer_amd.gene_pred_hmm_emitter import GenePredHMMEmitter
    from hmm_layer_amd.gene_pred_hmm_transitioner import GenePredMultiHMMTransitioner
    b, L, q = 3, 450, 71
    g = torch.Generator().manual_seed(12)
    cls = torch.softmax(2 * torch.randn((1, b, L, 15), generator=g), -1)
    nuc = torch.nn.functional.one_hot(torch.randint(0, 5, (1, b, L), generator=g), 5).float()
    x = torch.cat([cls, nuc], -1).to(DEV)
    em = GenePredHMMEmitter(**mct.CODONS, num_copies=5)
    em.build((1, b, L, 15))
    tr = GenePredMultiHMMTransitioner(k=5, initial_exon_len=200, initial_intron_len=4500, initial_ir_len=10000)
    cell = HmmCell([q], 15, em, tr).to(DEV)
    layer = MsaHmmLayer(cell, use_prior=False)
    layer.build(x.shape)
    table = cases.gene_classes(q)
    with torch.no_grad():
        got = layer.posterior_decode(x, state_class=table)
        assert cell.emitter[0].can_fuse(x)                               # the layer's E comes from the fused wide emitter
        A, pi, E = _engine_inputs(x, cell, None, False)
        gamma, ll = engine.posterior_walk(A, pi, E, mode=engine.POST_PROB, eps=cell.epsilon)
    torch.cuda.synchronize()
    assert got[0].is_cuda and got[0].dtype == torch.uint8 and tuple(got[0].shape) == (1, b, L)
    assert_classes(gamma, got, table, 6, "layer")
    want = engine.decode_posterior(gamma, table, 6)[0]
    sure = ref.decode(gamma.cpu().numpy(), table, 6)[2] > 2 * cases.tol(15)
    assert np.array_equal(got[0].cpu().numpy()[sure], want.cpu().numpy()[sure]) and torch.equal(got[2], ll)
    assert int(got[0].max()) > 0
