"""engine.posterior_decode / hmm_posterior_decode on the device: fused class posteriors and labels for up to 16 states.

The decode kernels share every instruction up to the gamma row with hmm_posterior's, so with the identity map the
result is held to engine.posterior(POST_PROB) BIT FOR BIT (label = lowest argmax, conf = max, loglik equal), in the
scan plan, in the windows and whole-sequence kernels of the clamp regime and for models routed per model.  With a class
map the class sums are fp32 in a fixed order and are held to fp64 sums of the engine's own gamma:
  |conf - ref| <= 2e-6    at most 15 fp32 additions of terms that sum to <= 1 (15 * 2^-24 = 9e-7), and the reference's
                          own fp64 rounding, on either side
  labels equal wherever the reference's margin between its two best classes exceeds 4e-6 (twice that); at most 1 % of
  a case's positions may lie inside the margin (random emissions: checked on the oracle alone in the CPU-side test
  below, which needs no device)
and to the fp64 oracle with the posteriors' own tolerance of 2e-5 per state (tests/test_engine_gpu.py::check_all):
  |conf - conf64| <= n_max * 2e-5, labels equal where the oracle's margin exceeds 2 * n_max * 2e-5, n_max the largest
  class."""
import numpy as np
import pytest
import torch

import posterior_decode_ref as ref
from hmm_layer_amd import engine
from hmm_layer_amd.MsaHMMLayer import MsaHmmLayer
from oracle import params, textbook
from test_engine_gpu import DEV, dev, gene7, rand_model
from test_layer_gpu import gene_setup

gpu = pytest.mark.gpu
OP = engine.OP_POSTERIOR
TAG = engine.DECODE_TAG
SHAPES = [(1, 1, 1), (1, 3, 3), (1, 3, 17), (1, 5, 33), (2, 3, 50), (2, 5, 333), (1, 17, 130)]
QS = [1, 2, 3, 4, 5, 7, 8, 12, 13, 15, 16]


def model(name, q, k, rng):
    """k models of q states -> A (k,q,q), pi (k,q): 'dense', or 'gene' (the compiled 7- / 15-state topologies)."""
    if name == "gene":
        A = np.stack([gene7() if q == 7 else params.intended_A15().numpy()] * k).astype(np.float32)
        pi = np.stack([rand_model(rng, q)[1] for _ in range(k)])
        return A, pi
    A, pi = zip(*(rand_model(rng, q) for _ in range(k)))
    return np.stack(A), np.stack(pi)


def emissions(rng, k, b, L, q):
    return (rng.random((k, b, L, q)) * 0.9 + 0.05).astype(np.float32)


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
    """Against fp64 class sums of the engine's own fp32 gamma (module docstring) -> share of positions skipped."""
    label, conf, _ = dec
    want, cref, margin = ref.decode(gamma, table, C)
    err = float(np.abs(conf - cref).max())
    sure = margin > 4e-6
    skipped = float((~sure).mean())
    print("%s: |conf - ref| max %.3g, positions within the margin %.4f" % (tag, err, skipped))
    assert err <= 2e-6, (tag, err)
    assert skipped <= 0.01, (tag, skipped)
    assert np.array_equal(label[sure], want[sure]), tag
    return skipped


# ---------------------------------------------------------------- 1. identity map, bit for bit

@gpu
@pytest.mark.parametrize("chunk", [16, 48])
@pytest.mark.parametrize("q", QS)
def test_identity_map_equals_posterior_bit_for_bit(q, chunk):
    rng = np.random.default_rng(1000 * q + chunk)
    with engine.option(engine.OPT_CHUNK, chunk):
        for name in ("dense", "gene") if q in (7, 15) else ("dense",):
            for k, b, L in SHAPES:
                A, pi = model(name, q, k, rng)
                E = emissions(rng, k, b, L, q)
                post, dec = both(A, pi, E)
                assert_identity(post, dec, (name, q, chunk, k, b, L))


@gpu
def test_block_lengths_optional_outputs():
    """The default chunk rule next to the forced chunk lengths of the test above, and the optional outputs.  (Chunk
    lengths are multiples of 16 in this build, so the scan plan's pair always walks 16-step blocks; the windows and
    the whole-sequence kernel walk 8-step blocks: both block lengths run in the clamp-regime tests.)"""
    rng = np.random.default_rng(7)
    A, pi = model("gene", 15, 1, rng)
    E = emissions(rng, 1, 5, 333, 15)
    for chunk in (0, 32):
        with engine.option(engine.OPT_CHUNK, chunk):
            T = engine.chunk_len(1, 5, 333, 15)
            assert chunk == 0 or T == chunk, T
            post, dec = both(A, pi, E)
            assert_identity(post, dec, ("T", T))
            _, nc = both(A, pi, E, want_conf=False)
            assert nc[1] is None and np.array_equal(nc[0], dec[0]) and np.array_equal(nc[2], dec[2])
    # loglik NULL, through the C ABI
    Ad, pid, Ed = dev(A), dev(pi), dev(E)
    label = torch.full((1, 5, 333), 255, dtype=torch.uint8, device=DEV)
    need = engine.lib().hmm_workspace_bytes(OP, 1, 5, 333, 15)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    rc = engine.lib().hmm_posterior_decode(Ad.data_ptr(), pid.data_ptr(), Ed.data_ptr(), 1, 5, 333, 15, engine.EPS, None, 15,
                                           label.data_ptr(), None, None, ws.data_ptr(), need,
                                           torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    with engine.option(engine.OPT_CHUNK, 0):
        post, dec = both(A, pi, E)
    assert rc == 0 and np.array_equal(label.cpu().numpy(), dec[0])


# ---------------------------------------------------------------- 2. class maps

def class_cases():
    rng = np.random.default_rng(2)
    cases = [("gene15-5", "gene", 15, ref.GENE_CLASSES, 5)]
    for q, C in ((15, 1), (16, 2), (13, 5), (16, 16), (7, 2), (5, 5)):
        cases.append(("dense%d-%d" % (q, C), "dense", q, ref.random_map(rng, q, C), C))
    cases.append(("dense12-empty", "dense", 12, ref.random_map(rng, 12, 5, empty=2), 5))
    cases.append(("gene15-empty0", "gene", 15, [c + 1 for c in ref.GENE_CLASSES], 6))
    return cases


@gpu
@pytest.mark.parametrize("case", class_cases(), ids=lambda c: c[0])
def test_class_maps_against_fp64_sums_of_the_engines_gamma(case):
    tag, name, q, table, C = case
    rng = np.random.default_rng(len(tag) + q)
    for chunk, (k, b, L) in ((16, (2, 5, 333)), (48, (1, 17, 130)), (16, (1, 3, 17))):
        with engine.option(engine.OPT_CHUNK, chunk):
            A, pi = model(name, q, k, rng)
            E = emissions(rng, k, b, L, q)
            for tab in (table, torch.tensor(table, dtype=torch.int32), torch.tensor(table, device=DEV)):
                post, dec = both(A, pi, E, tab, C)
                assert_classes(post[0], dec, table, C, (tag, chunk, k, b, L))
                assert np.array_equal(dec[2], post[1])
                unused = sorted(set(range(C)) - set(table))              # an empty class sums to zero: never the label
                assert dec[0].max() < C and not np.isin(dec[0], unused).any()


@gpu
def test_uniform_model_ties_go_to_class_zero():
    """Uniform A, pi and E: every state has the same posterior, so classes of equal size tie exactly."""
    for q, table, C in ((15, None, None), (15, [i % 5 for i in range(15)], 5), (16, [i // 4 for i in range(16)], 4),
                        (6, [2, 1, 0, 2, 1, 0], 3), (1, None, None)):
        A = np.full((1, q, q), 1 / q, dtype=np.float32)
        pi = np.full((1, q), 1 / q, dtype=np.float32)
        E = np.full((1, 3, 130, q), 0.25, dtype=np.float32)
        _, (label, conf, _) = both(A, pi, E, table, C)
        assert not label.any(), (q, table)
        assert np.allclose(conf, 1 / (C or q), rtol=1e-6)


def test_reference_margin_is_rarely_small():
    """The share of positions that the class-map test may skip, on the fp64 oracle alone (no device): random
    emissions put far fewer than 1 % of the positions within 4e-6 of a tie."""
    rng = np.random.default_rng(3)
    A = params.intended_A15().numpy().astype(np.float32)
    pi = np.full(15, 1 / 15, dtype=np.float32)
    E = emissions(rng, 1, 5, 333, 15)[0]
    g64, _ = textbook.posterior(A, pi, E)
    for table, C in ((ref.GENE_CLASSES, 5), (ref.random_map(rng, 15, 2), 2), (list(range(15)), 15)):
        assert (ref.decode(g64, table, C)[2] <= 4e-6).mean() < 0.01


# ---------------------------------------------------------------- 3. fp64 oracle

@gpu
@pytest.mark.parametrize("name,q,table,C,nmax", [("gene", 15, ref.GENE_CLASSES, 5, ref.GENE_NMAX),
                                                 ("gene", 15, None, 15, 1), ("gene", 7, [0, 1, 1, 1, 2, 2, 2], 3, 3),
                                                 ("dense", 16, [i % 4 for i in range(16)], 4, 4)])
def test_against_the_fp64_oracle(name, q, table, C, nmax):
    rng = np.random.default_rng(30 + q + C)
    k, b, L = 1, 5, 333
    A, pi = model(name, q, k, rng)
    E = emissions(rng, k, b, L, q)
    with engine.option(engine.OPT_CHUNK, 48):
        _, (label, conf, ll) = both(A, pi, E, table, C)
    g64, ll64 = textbook.posterior(A[0], pi[0], E[0])
    want, c64, margin = ref.decode(g64, table, C)
    err = float(np.abs(conf[0] - c64).max())
    sure = margin > 2 * nmax * 2e-5
    print("|conf - conf64| max %.3g (bound %.3g), positions within the margin %.4f" % (err, nmax * 2e-5, (~sure).mean()))
    assert err <= nmax * 2e-5
    assert np.array_equal(label[0][sure], want[sure])
    assert np.all(np.abs(ll[0] - ll64) <= 1e-6 * np.abs(ll64) + 2e-4)


# ---------------------------------------------------------------- 4. the clamp regime

def clamp_case():
    """The gene model, chunks of 16: sequence 1 has one stretch that state 9 (EI1, left after one step) emits alone —
    a window —, sequence 3 has zeros all over — recomputed whole —, the others stay on the scan."""
    rng = np.random.default_rng(77)
    A = params.intended_A15().numpy().astype(np.float32)[None]
    pi = np.full((1, 15), 1 / 15, dtype=np.float32)
    b, L = 5, 1500
    E = emissions(rng, 1, b, L, 15)
    E[0, 1, 700:704, :] = 0.0
    E[0, 1, 700:704, 9] = 0.5
    hard = E[0, 3]
    hard[rng.random(hard.shape) < 0.25] = 0.0
    return A, pi, E


@gpu
def test_clamp_regime_windows_and_whole_sequences():
    A, pi, E = clamp_case()
    dims = (1,) + E.shape[1:]
    with engine.option(engine.OPT_CHUNK, 16):
        post, dec = both(A, pi, E)
        n_post, n_dec = engine.exact_count(OP, dims), engine.exact_count(OP, dims, tag=TAG)
        d_post, d_dec = engine.exact_detail(dims), engine.exact_detail(dims, tag=TAG)
        print("routing", d_dec)
        assert n_dec > 0 and n_dec == n_post and d_dec == d_post
        assert d_dec["window_sequences"] >= 1 and d_dec["whole"] >= 1 and d_dec["routed"] < dims[1]
        assert engine.window_table(dims, 1, tag=TAG)["windows"] == engine.window_table(dims, 1)["windows"]
        assert_identity(post, dec, "auto")
        post, dec = both(A, pi, E, ref.GENE_CLASSES, 5)
        assert_classes(post[0], dec, ref.GENE_CLASSES, 5, "auto, classes")
        for how in (engine.EXACT_ALWAYS, engine.EXACT_ALWAYS_NARROW, engine.EXACT_OFF):
            with engine.option(engine.OPT_EXACT, how):
                post, dec = both(A, pi, E)
                n = engine.exact_count(OP, dims, tag=TAG)
                assert n == engine.exact_count(OP, dims) == (0 if how == engine.EXACT_OFF else dims[1]), (how, n)
                assert_identity(post, dec, ("exact mode", how))


@gpu
def test_models_routed_per_model():
    """A cycle (periodic) and A = I next to a primitive model in one call: k_topo_check sends the first two to the
    whole-sequence kernel, waves straddle the models."""
    rng = np.random.default_rng(41)
    q, b, L = 5, 3, 130
    A = np.stack([np.roll(np.eye(q, dtype=np.float32), 1, axis=1), rand_model(rng, q)[0], np.eye(q, dtype=np.float32)])
    pi = np.stack([rand_model(rng, q)[1] for _ in range(3)])
    E = emissions(rng, 3, b, L, q)
    with engine.option(engine.OPT_CHUNK, 16):
        post, dec = both(A, pi, E)
        assert engine.exact_count(OP, (3, b, L, q), tag=TAG) == engine.exact_count(OP, (3, b, L, q)) == 2 * b
        assert_identity(post, dec, "routed models")
        table = [0, 1, 1, 0, 2]
        post, dec = both(A, pi, E, table, 3)
        assert_classes(post[0], dec, table, 3, "routed models, classes")


# ---------------------------------------------------------------- 5. determinism and capture

@gpu
def test_repeated_calls_are_bit_identical():
    A, pi, E = clamp_case()
    with engine.option(engine.OPT_CHUNK, 16):
        _, first = both(A, pi, E, ref.GENE_CLASSES, 5)
        _, second = both(A, pi, E, ref.GENE_CLASSES, 5)
    for x, y in zip(first, second):
        assert np.array_equal(x, y)


@gpu
def test_graph_capture_keeps_its_class_table():
    rng = np.random.default_rng(21)
    A = params.intended_A15().to(DEV)[None]
    pi = torch.full((15,), 1 / 15, device=DEV)
    E = torch.rand((1, 8, 3000, 15), device=DEV) * 0.9 + 0.05            # one batch group
    table = list(ref.GENE_CLASSES)
    engine.posterior_decode(A, pi, E, table)                            # warm-up: the workspace is allocated here
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        engine.posterior_decode(A, pi, E, table)                        # (this stream's workspace)
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            label, conf, ll = engine.posterior_decode(A, pi, E, table)
    E2 = torch.rand((1, 8, 3000, 15), device=DEV) * 0.9 + 0.05
    E.copy_(E2)
    for i in range(15):                                                 # the caller's list changes after the capture
        table[i] = 0
    g.replay()
    torch.cuda.synchronize()
    want = engine.posterior_decode(A, pi, E2, ref.GENE_CLASSES)
    torch.cuda.synchronize()
    assert torch.equal(label, want[0]) and torch.equal(conf, want[1]) and torch.equal(ll, want[2])
    assert int(label.max()) > 0


# ---------------------------------------------------------------- 6. above 16 states: posterior + torch ops

@gpu
@pytest.mark.parametrize("q", [29, 24])
def test_fallback_above_sixteen_states(q):
    rng = np.random.default_rng(q)
    if q == 29:
        import logab_sweep
        A = logab_sweep.gene_model(2)[None]
        table, C = [0] + [1 + (i % 14) // 3 for i in range(28)], 6
    else:
        A = rand_model(rng, q)[0][None]
        table, C = ref.random_map(rng, q, 20), 20
    pi = np.full((1, q), 1 / q, dtype=np.float32)
    E = emissions(rng, 1, 3, 130, q)
    for tab, CC in ((None, None), (table, C)):
        post, dec = both(A, pi, E, tab, CC)
        if tab is None:
            assert_identity(post, dec, q)
        else:
            assert_classes(post[0], dec, table, C, "q=%d" % q)
            assert np.array_equal(dec[2], post[1])
    A1 = np.full((1, q, q), 1 / q, dtype=np.float32)
    _, (label, _, _) = both(A1, pi, np.full((1, 2, 40, q), 0.25, dtype=np.float32))
    assert not label.any()


# ---------------------------------------------------------------- 7. the layer

@gpu
def test_layer_posterior_decode_fused_emitter_path():
    b, L = 3, 700
    cell, x, A, pi, E = gene_setup(b, L, seed=5)
    layer = MsaHmmLayer(cell, use_prior=False)
    with torch.no_grad():
        probs, ll = layer.state_posterior_probs(x)
        label, conf, lld = layer.posterior_decode(x, state_class=ref.GENE_CLASSES)
        ident = layer.posterior_decode(x)
    torch.cuda.synchronize()
    assert label.is_cuda and label.dtype == torch.uint8 and tuple(label.shape) == (1, b, L)
    gamma = probs.cpu().numpy()
    assert_classes(gamma, (label.cpu().numpy(), conf.cpu().numpy(), None), ref.GENE_CLASSES, 5, "layer")
    assert torch.equal(lld, ll)
    assert_identity((gamma, ll.cpu().numpy()), tuple(t.cpu().numpy() for t in ident), "layer, identity")
    with pytest.raises(ValueError, match="state_posterior_log_probs"):
        layer.posterior_decode(x.clone().requires_grad_(True))
