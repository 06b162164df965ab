"""engine.posterior_decode / hmm_posterior_decode_mid on the device: fused class posteriors and labels for 17..64
states, on the chunked scan (32- and 64-lane rows) and on the one-wave-per-sequence walk.

The decode kernels share every instruction up to the gamma row with hmm_posterior's, so with the identity map the
result is held to engine.posterior(POST_PROB) BIT FOR BIT (label = lowest argmax, conf = max, loglik equal) on every
path.  With a class map the class sums are fp32 in state order and are held to fp64 sums of the engine's own gamma
(posterior_decode_ref.decode), n the largest class of the map:
  |conf - ref| <= tol(n) = 2e-6 * max(1, (n - 1) / 15)   the q <= 16 test's bound (15 additions * 2^-24 = 9e-7,
                          doubled for the reference side), scaled with the number of additions
  labels equal wherever the reference's margin between its two best classes exceeds 2 tol(n); at most 1 % of a case's
  positions may lie inside the margin (checked on the oracle alone in tests/test_posterior_decode_mid_cpu.py)
and to the fp64 oracle with the posteriors' own tolerance of 2e-5 per state:
  |conf - conf64| <= n * 2e-5, labels equal where the oracle's margin exceeds 2 n * 2e-5, at most 2 % inside it."""
import ctypes

import numpy as np
import pytest
import torch

import memory_contract_table as mct
import posterior_decode_mid_cases as cases
import posterior_decode_ref as ref
from hmm_layer_amd import engine
from hmm_layer_amd.MsaHMMLayer import MsaHmmLayer, _engine_inputs
from oracle import textbook
from test_engine_gpu import DEV, dev, rand_model

gpu = pytest.mark.gpu
OP = engine.OP_POSTERIOR
TAG = engine.DECODE_TAG
SHAPES = [(1, 1, 1), (1, 3, 3), (1, 3, 17), (1, 5, 33), (2, 3, 50), (2, 5, 333), (1, 17, 130)]
SHAPES64 = [(1, 2, 300), (2, 3, 530),                   # 33..64 states: the 64-lane scan (few long sequences)
            (1, 3, 37), (1, 97, 20)]                    # ... and the walk alone (short, or more than 96 sequences)
MODELS = [("dense", 17), ("dense", 24), ("gene", 29), ("dense", 29), ("dense", 32), ("dense", 33), ("dense", 40),
          ("gene", 43), ("dense", 48), ("gene", 57), ("dense", 64)]
RING = 64                                               # MQ_RING: each wave of the walk drains its ring when 64 rows are in it
WALK_LENGTHS = (1, 2, 63, 64, 65, 130, 2 * RING - 1, 2 * RING, 2 * RING + 1, 4 * RING + 3)
WALKS = [("dense", 24), ("dense", 40), ("dense", 64), ("gene", 29), ("gene", 43), ("gene", 57)]   # QB 32 48 64, D 4 4 8


def both(A, pi, E, table=None, C=None, want_conf=True):
    """-> (gamma, loglik) of engine.posterior and (label, conf, loglik) of engine.posterior_decode, as numpy."""
    A, pi, E = dev(A), dev(pi), dev(E)
    gamma, ll = engine.posterior(A, pi, E)
    label, conf, lld = engine.posterior_decode(A, pi, E, state_class=table, num_classes=C, want_conf=want_conf)
    torch.cuda.synchronize()
    assert label.dtype == torch.uint8 and label.shape == E.shape[:3] and lld.dtype == torch.float64
    assert (conf is None) if not want_conf else (conf.dtype == torch.float32 and conf.shape == E.shape[:3])
    return (gamma.cpu().numpy(), ll.cpu().numpy()), (label.cpu().numpy(), None if conf is None else conf.cpu().numpy(),
                                                     lld.cpu().numpy())


def assert_identity(post, dec, tag):
    (gamma, ll), (label, conf, lld) = post, dec
    assert np.array_equal(label, gamma.argmax(-1).astype(np.uint8)), tag       # numpy: the first maximal index
    if conf is not None:
        assert np.array_equal(conf, gamma.max(-1)), tag
    assert np.array_equal(lld, ll), tag


def assert_classes(gamma, dec, table, C, tag):
    """Against fp64 class sums of the engine's own fp32 gamma (module docstring)."""
    label, conf, _ = dec
    n = cases.largest_class(table, C)
    want, cref, margin = ref.decode(gamma, table, C)
    err = float(np.abs(conf - cref).max())
    sure = margin > 2 * cases.tol(n)
    skipped = float((~sure).mean())
    print("%s: n = %d, |conf - ref| max %.3g (bound %.3g), positions within the margin %.5f"
          % (tag, n, err, cases.tol(n), skipped))
    assert err <= cases.tol(n), (tag, err)
    assert skipped <= cases.MARGIN_CAP, (tag, skipped)
    assert np.array_equal(label[sure], want[sure]), tag
    unused = sorted(set(range(C)) - set(table))                  # an empty class sums to zero: never the label
    assert label.max() < C and not np.isin(label, unused).any(), tag


@pytest.fixture
def fused_only(monkeypatch):
    """engine.posterior_decode must not compose: the posterior is out of reach while the fixture holds."""
    real = engine.posterior

    def refuse(*a, **kw):
        raise AssertionError("posterior_decode composed engine.posterior")
    monkeypatch.setattr(engine, "posterior", refuse)
    return real


# ---------------------------------------------------------------- 1. identity map, bit for bit

@gpu
@pytest.mark.parametrize("chunk", [0, 16, 48])
@pytest.mark.parametrize("name,q", MODELS, ids=lambda v: str(v))
def test_identity_map_equals_posterior_bit_for_bit(name, q, chunk):
    rng = np.random.default_rng(1000 * q + chunk + (name == "gene"))
    dense_opts = (0, 1) if name == "gene" and chunk == 16 else (0,)
    with engine.option(engine.OPT_CHUNK, chunk):
        for k, b, L in SHAPES + (SHAPES64 if q > 32 else []):
            A, pi = cases.model(name, q, k, rng)
            E = cases.emissions(rng, k, b, L, q)
            for force in dense_opts:                                       # the gene models: sparse and dense kernels
                with engine.option(engine.OPT_FORCE_DENSE, force):
                    post, dec = both(A, pi, E)
                    assert_identity(post, dec, (name, q, chunk, k, b, L, force))


@gpu
def test_optional_outputs():
    rng = np.random.default_rng(7)
    for name, q, (k, b, L) in (("gene", 29, (1, 5, 333)), ("dense", 40, (1, 2, 300)), ("gene", 43, (1, 3, 37))):
        A, pi = cases.model(name, q, k, rng)
        E = cases.emissions(rng, k, b, L, q)
        post, dec = both(A, pi, E)
        assert_identity(post, dec, (name, q))
        _, nc = both(A, pi, E, want_conf=False)
        assert nc[1] is None and np.array_equal(nc[0], dec[0]) and np.array_equal(nc[2], dec[2])
        # loglik NULL (and conf NULL), through the C ABI
        Ad, pid, Ed = dev(A), dev(pi), dev(E)
        label = torch.full((k, b, L), 255, dtype=torch.uint8, device=DEV)
        need = engine.lib().hmm_posterior_decode_mid_workspace_bytes(k, b, L, q)
        ws = torch.empty(need, dtype=torch.uint8, device=DEV)
        rc = engine.lib().hmm_posterior_decode_mid(Ad.data_ptr(), pid.data_ptr(), Ed.data_ptr(), k, b, L, q, engine.EPS,
                                                   None, q, label.data_ptr(), None, None, ws.data_ptr(), need,
                                                   torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert rc == 0 and np.array_equal(label.cpu().numpy(), dec[0])


# ---------------------------------------------------------------- 2. the serial walk, every instantiation

@gpu
@pytest.mark.parametrize("name,q", WALKS, ids=lambda v: str(v))
def test_walk_instantiations_under_exact_always(name, q):
    rng = np.random.default_rng(50 + q)
    table = cases.gene_classes(q) if name == "gene" else cases.random_map(rng, q, 5)
    with engine.option(engine.OPT_EXACT, engine.EXACT_ALWAYS):
        for L in WALK_LENGTHS:
            A, pi = cases.model(name, q, 1, rng)
            E = cases.emissions(rng, 1, 3, L, q)
            post, dec = both(A, pi, E)
            if q <= 32:                                        # (above, these shapes are the walk's whatever the option)
                assert engine.exact_count(OP, (1, 3, L, q), tag=TAG) == engine.exact_count(OP, (1, 3, L, q)) == 3
            assert_identity(post, dec, (name, q, L))
        post, dec = both(A, pi, E, table, max(table) + 1)      # (the last, longest shape)
        assert_classes(post[0], dec, table, max(table) + 1, ("walk", name, q))
        assert np.array_equal(dec[2], post[1])


@gpu
def test_mixed_batch_scan_and_walk_side_by_side():
    """A six-position all-zero stretch in one sequence of a two-copy gene batch, chunks of 16: the certificate sends
    that sequence to the walk, the others stay on the scan."""
    k, b, L, q = 1, 3, 100, 29
    A, pi = mct.models(("g29",))
    E = mct.emissions(("decode_mid", ("g29",)), k, b, L, q, stretch=True)
    with engine.option(engine.OPT_CHUNK, 16), engine.option(engine.OPT_EXACT, engine.EXACT_AUTO):
        post, dec = both(A, pi, E)
        n = engine.exact_count(OP, (k, b, L, q), tag=TAG)
        assert 0 < n < k * b and n == engine.exact_count(OP, (k, b, L, q)), n
        assert_identity(post, dec, "mixed")
        table = cases.gene_classes(q)
        post, dec = both(A, pi, E, table, 6)
        assert_classes(post[0], dec, table, 6, "mixed, classes")


@gpu
def test_models_routed_per_model():
    """A reducible model (two blocks that never meet) next to a primitive one in one call: the device sends the
    first to the walk, waves straddle the models."""
    rng = np.random.default_rng(41)
    q, b, L = 24, 3, 130
    A0 = np.zeros((q, q), dtype=np.float32)
    A0[:12, :12] = rand_model(rng, 12)[0]
    A0[12:, 12:] = rand_model(rng, 12)[0]
    A = np.stack([A0, rand_model(rng, q)[0]])
    pi = np.stack([rand_model(rng, q)[1] for _ in range(2)])
    E = cases.emissions(rng, 2, b, L, q)
    with engine.option(engine.OPT_CHUNK, 16):
        post, dec = both(A, pi, E)
        assert engine.exact_count(OP, (2, b, L, q), tag=TAG) == engine.exact_count(OP, (2, b, L, q)) == b
        assert_identity(post, dec, "routed model")
        table = cases.random_map(rng, q, 4)
        post, dec = both(A, pi, E, table, 4)
        assert_classes(post[0], dec, table, 4, "routed model, classes")


# ---------------------------------------------------------------- 3. class maps

@gpu
@pytest.mark.parametrize("case", cases.class_cases(), ids=lambda c: c[0])
def test_class_maps_against_fp64_sums_of_the_engines_gamma(case, fused_only):
    tag, name, q, table, C, seed = case
    for chunk, shape in cases.CLASS_SHAPES:
        A, pi, E = cases.class_inputs(case, shape)
        with engine.option(engine.OPT_CHUNK, chunk):
            gamma, ll = fused_only(dev(A), dev(pi), dev(E))
            for tab in (table, torch.tensor(table, dtype=torch.int32, device=DEV)):
                label, conf, lld = engine.posterior_decode(dev(A), dev(pi), dev(E), tab, C)
                torch.cuda.synchronize()
                assert_classes(gamma.cpu().numpy(), (label.cpu().numpy(), conf.cpu().numpy(), None), table, C,
                               (tag, chunk) + shape)
                assert torch.equal(lld, ll)


@gpu
def test_uniform_model_ties_go_to_class_zero():
    """Uniform A, pi and E: every state has the same posterior, so classes of equal size tie exactly."""
    for q, table, C in ((29, None, None), (30, [i % 5 for i in range(30)], 5), (64, [i // 4 for i in range(64)], 16),
                        (64, None, None), (40, [3 - i % 4 for i in range(40)], 4)):
        A = np.full((1, q, q), 1 / q, dtype=np.float32)
        pi = np.full((1, q), 1 / q, dtype=np.float32)
        for b, L in ((3, 130), (2, 300)):                                   # (64 states: the walk, the 64-lane scan)
            E = np.full((1, b, L, q), 0.25, dtype=np.float32)
            _, (label, conf, _) = both(A, pi, E, table, C)
            assert not label.any(), (q, table)
            assert np.allclose(conf, 1 / (C or q), rtol=1e-5)


# ---------------------------------------------------------------- 4. fp64 oracle

@gpu
@pytest.mark.parametrize("case", cases.oracle_cases(), ids=lambda c: c[0])
def test_against_the_fp64_oracle(case):
    tag, name, q, table, C, seed = case
    n = 1 if table is None else cases.largest_class(table, C)
    A, pi, E = cases.oracle_inputs(case)
    with engine.option(engine.OPT_CHUNK, 48):
        _, (label, conf, ll) = both(A, pi, E, table, C)
    g64, ll64 = textbook.posterior(A[0], pi[0], E[0])
    want, c64, margin = ref.decode(g64, table, C)
    err = float(np.abs(conf[0] - c64).max())
    sure = margin > 2 * n * cases.STATE_TOL
    print("%s: |conf - conf64| max %.3g (bound %.3g), positions within the margin %.4f"
          % (tag, err, n * cases.STATE_TOL, (~sure).mean()))
    assert err <= n * cases.STATE_TOL
    assert (~sure).mean() <= cases.ORACLE_CAP
    assert np.array_equal(label[0][sure], want[sure])
    assert np.all(np.abs(ll[0] - ll64) <= 1e-6 * np.abs(ll64) + 2e-4)


# ---------------------------------------------------------------- 5. determinism and capture

@gpu
@pytest.mark.parametrize("exact", [engine.EXACT_AUTO, engine.EXACT_ALWAYS])
def test_repeated_calls_are_bit_identical_on_a_dirtied_workspace(exact):
    k, b, L, q = 1, 3, 100, 29
    A, pi = mct.models(("g29",))
    E = mct.emissions(("decode_mid", ("g29",)), k, b, L, q, stretch=True)
    table = cases.gene_classes(q)
    A, pi, E = dev(A), dev(pi), dev(E)
    with engine.option(engine.OPT_CHUNK, 16), engine.option(engine.OPT_EXACT, exact):
        first = engine.posterior_decode(A, pi, E, table, 6)
        torch.cuda.synchronize()
        first = [t.clone() for t in first]
        ws = engine._workspace(torch.device(DEV), 0, TAG)
        ws.fill_(0xA5)                                                  # (every float a large negative number)
        second = engine.posterior_decode(A, pi, E, table, 6)
        torch.cuda.synchronize()
    for x, y in zip(first, second):
        assert torch.equal(x, y)


@gpu
@pytest.mark.parametrize("exact", [engine.EXACT_AUTO, engine.EXACT_ALWAYS])
def test_graph_capture_keeps_its_class_table(exact):
    q = 29
    A = dev(cases.gene(q)[0])[None]
    pi = dev(cases.gene(q)[1])
    shape = (1, 4, 600, q)
    E = 0.05 + 0.9 * torch.rand(shape, device=DEV) ** 4
    classes = cases.gene_classes(q)
    table = list(classes)
    with engine.option(engine.OPT_EXACT, exact):
        engine.posterior_decode(A, pi, E, table)                        # warm-up: the workspace is allocated here
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            engine.posterior_decode(A, pi, E, table)                    # (this stream's workspace)
            torch.cuda.synchronize()
            with torch.cuda.graph(g, stream=s):
                label, conf, ll = engine.posterior_decode(A, pi, E, table)
        E2 = 0.05 + 0.9 * torch.rand(shape, device=DEV) ** 4
        E.copy_(E2)
        for i in range(q):                                              # the caller's list changes after the capture
            table[i] = 0
        g.replay()
        torch.cuda.synchronize()
        want = engine.posterior_decode(A, pi, E2, classes)
        torch.cuda.synchronize()
    assert torch.equal(label, want[0]) and torch.equal(conf, want[1]) and torch.equal(ll, want[2])
    assert int(label.max()) > 0


# ---------------------------------------------------------------- 6. routing of the wrapper

@gpu
@pytest.mark.parametrize("q", [29, 43])
def test_wrapper_takes_the_fused_path(q, fused_only):
    rng = np.random.default_rng(q)
    A, pi = cases.model("gene", q, 1, rng)
    E = cases.emissions(rng, 1, 3, 130, q)
    table = cases.gene_classes(q)
    for tab, C in ((None, None), (table, 6)):
        label, conf, ll = engine.posterior_decode(dev(A), dev(pi), dev(E), tab, C)
        torch.cuda.synchronize()
        gamma, llp = fused_only(dev(A), dev(pi), dev(E))
        dec = (label.cpu().numpy(), conf.cpu().numpy(), ll.cpu().numpy())
        if tab is None:
            assert_identity((gamma.cpu().numpy(), llp.cpu().numpy()), dec, q)
        else:
            assert_classes(gamma.cpu().numpy(), dec, table, 6, "q=%d" % q)


@gpu
def test_wrapper_composes_above_sixteen_classes(monkeypatch):
    rng = np.random.default_rng(24)
    q = 24
    A, pi = cases.model("dense", q, 1, rng)
    E = cases.emissions(rng, 1, 3, 130, q)
    table = cases.random_map(rng, q, 20)
    calls = []
    real = engine.posterior
    monkeypatch.setattr(engine, "posterior", lambda *a, **kw: calls.append(1) or real(*a, **kw))
    label, conf, ll = engine.posterior_decode(dev(A), dev(pi), dev(E), table, 20)
    assert calls == [1]
    gamma, _ = real(dev(A), dev(pi), dev(E))
    want, cref, _ = ref.decode(gamma.cpu().numpy(), table, 20)
    assert np.abs(conf.cpu().numpy() - cref).max() <= 2e-6 and int(label.max()) < 20


# ---------------------------------------------------------------- 7. the layer

@gpu
def test_layer_posterior_decode_two_copy_gene_model():
    from hmm_layer_amd.MsaHmmCell import HmmCell
    from hmm_layer_amd.gene_pred_hmm_emitter import GenePredHMMEmitter
    from hmm_layer_amd.gene_pred_hmm_transitioner import GenePredMultiHMMTransitioner
    b, L = 3, 450
    g = torch.Generator().manual_seed(12)
    cls = torch.softmax(2 * torch.randn((1, b, L, 15), generator=g), -1)
    nuc = torch.nn.functional.one_hot(torch.randint(0, 5, (1, b, L), generator=g), 5).float()
    x = torch.cat([cls, nuc], -1).to(DEV)
    em = GenePredHMMEmitter(**mct.CODONS, num_copies=2)
    em.build((1, b, L, 15))
    tr = GenePredMultiHMMTransitioner(k=2, initial_exon_len=200, initial_intron_len=4500, initial_ir_len=10000)
    cell = HmmCell([29], 15, em, tr).to(DEV)
    layer = MsaHmmLayer(cell, use_prior=False)
    layer.build(x.shape)
    table = cases.gene_classes(29)
    with torch.no_grad():
        got = layer.posterior_decode(x, state_class=table)
        ident = layer.posterior_decode(x)
        assert cell.emitter[0].can_fuse(x)                               # the layer's E comes from the fused emitter
        A, pi, E = _engine_inputs(x, cell, None, False)
        want = engine.posterior_decode(A, pi, E, table, eps=cell.epsilon)
        want_ident = engine.posterior_decode(A, pi, E, eps=cell.epsilon)
    torch.cuda.synchronize()
    assert got[0].is_cuda and got[0].dtype == torch.uint8 and tuple(got[0].shape) == (1, b, L)
    for x_, y_ in zip(got + ident, want + want_ident):
        assert torch.equal(x_, y_)
    assert int(got[0].max()) > 0
