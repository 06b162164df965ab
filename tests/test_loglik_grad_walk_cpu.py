"""hmm_loglik_grad_walk (log-likelihoods and their gradients by the per-sequence walk with the sparse step, 65..256
states) without a device: the argument checks of the C ABI in the order the header states, the state and workspace
queries, the typed symbols, the wrappers' refusals; from the fp64 oracle and its fp32 twin alone, that every case of
tests/loglik_grad_walk_cases.py can carry the comparison of tests/test_loglik_grad_walk_gpu.py; and the proof that the
gene transitioner never reads the gradient of an absent edge, which is what makes dA on the support of A sound."""
import numpy as np
import pytest
import torch

import loglik_grad_walk_cases as wc
from hmm_layer_amd import autograd
from hmm_layer_amd import build as hbuild
from hmm_layer_amd import engine
from hmm_layer_amd.gene_pred_hmm_transitioner import GenePredMultiHMMTransitioner

SPECS = wc.all_specs() + [wc.refused_case()]


@pytest.fixture(scope="module")
def lib():
    hbuild.build()
    return engine.lib()


def test_state_range(lib):
    assert lib.hmm_loglik_grad_walk_min_states() == 65 and lib.hmm_loglik_grad_walk_max_states() == 256


def test_validation_order_without_device(lib):
    # shape, q outside 65..256, pointers, then the workspace; nothing here reaches a HIP call
    p = 0x10000                                                                 # never dereferenced
    eps, big = 1e-16, 1 << 40
    k, b, L, q = 2, 3, 17, 71
    f = lib.hmm_loglik_grad_walk
    assert f(None, None, None, k, b, 0, q, eps, None, None, None, None, None, None, 0, None) == -1
    assert f(None, None, None, k, 0, L, 64, eps, None, None, None, None, None, None, 0, None) == -1
    assert f(None, None, None, 0, b, L, 257, eps, None, None, None, None, None, None, 0, None) == -1
    for bad_q in (1, 16, 64, 257, 4096):
        assert f(None, None, None, k, b, L, bad_q, eps, None, None, None, None, None, None, 0, None) == -2, bad_q
    for hole in range(4):                                                       # A, pi, E, workspace
        a = [p, p, p, p]
        a[hole] = None
        assert f(a[0], a[1], a[2], k, b, L, q, eps, None, p, p, p, p, a[3], big, None) == -3, hole
    for grads in ((p, None, None), (None, p, None), (None, None, p), (p, p, None), (p, None, p), (None, p, p)):
        assert f(p, p, p, k, b, L, q, eps, None, *grads, p, p, 0, None) == -3, grads       # one or two of the three
    assert f(p, p, p, k, b, L, q, eps, p, None, None, None, None, p, 0, None) == -3         # nothing asked for
    need = lib.hmm_loglik_grad_walk_workspace_bytes(k, b, L, q)
    for grads, ll in (((p, p, p), p), ((p, p, p), None), ((None, None, None), p)):         # grad_loglik, loglik NULL-able
        assert f(p, p, p, k, b, L, q, eps, None, *grads, ll, p, need - 1, None) == -4
        assert f(p, p, p, k, b, L, q, eps, p, *grads, ll, p + 1, big, None) == -4
    r = lib.hmm_loglik_grad_walk_refused
    assert r(k, b, 0, q, p, big) == -1 and r(k, b, L, 64, p, big) == -2 and r(k, b, L, q, None, big) == -3
    assert r(k, b, L, q, p, need - 1) == -4


def test_workspace_queries(lib):
    query = lib.hmm_loglik_grad_walk_workspace_bytes
    for k, b, L, q in ((1, 1, 1, 65), (2, 3, 17, 71), (1, 5, 333, 128), (1, 2, 300, 129), (2, 3, 530, 256),
                      (1, 1024, 1000, 253)):
        w = query(k, b, L, q)
        assert w > 0 and w % 256 == 0 and w == query(k, b, 7 * L + 1, q), (k, b, L, q)   # no part grows with L
        assert w >= 4 * k * b * 10 * 64 * ((q + 63) // 64)                             # the sequences' accumulators
    for q in (1, 16, 64, 257, 1027):
        assert query(2, 3, 17, q) == 0, q
    assert query(0, 3, 17, 71) == 0 and query(2, 0, 17, 71) == 0 and query(2, 3, 0, 71) == 0
    assert query(1, 1024, 10000, 253) < 64 << 20


def test_pays_is_zero_outside_the_range(lib):
    for dims in ((1, 32, 10000, 64), (1, 32, 10000, 257), (0, 32, 10000, 71), (1, 32, 0, 71), (1, 0, 10, 127)):
        assert lib.hmm_loglik_grad_walk_pays(*dims) == 0, dims
    # the measured rule (profiles/loglik_grad_walk.json): every measured cell pays, 1 / 32 / 1024 sequences at 71, 127
    # and 253 states; more than 1024 sequences per call were not measured
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "loglik_grad_walk.json")) as fh:
        prof = json.load(fh)
    assert {(q, b) for q in prof["pays"] for b in prof["pays"][q]} == {(str(q), str(b)) for q in wc.GENE_Q for b in (1, 32, 1024)}
    for q, cells in prof["pays"].items():
        for b, cell in cells.items():
            assert cell["pays"] == int(cell["grad_large_over_walk"] >= prof["margin"]) == 1
            assert lib.hmm_loglik_grad_walk_pays(1, int(b), prof["L"], int(q)) == cell["pays"], (q, b)
    for q in (65, 71, 128, 129, 256):
        for k, b in ((1, 1), (2, 512), (3, 5)):
            assert lib.hmm_loglik_grad_walk_pays(k, b, 130, q) == 1, (k, b, q)
        for k, b in ((1, 1025), (2, 513), (1, 4096)):
            assert lib.hmm_loglik_grad_walk_pays(k, b, 10000, q) == 0, (k, b, q)


def test_symbols_are_typed(lib):
    assert set(engine.LOGLIK_GRAD_WALK_SIGNATURES) == {
        "hmm_loglik_grad_walk_min_states", "hmm_loglik_grad_walk_max_states", "hmm_loglik_grad_walk_workspace_bytes",
        "hmm_loglik_grad_walk_pays", "hmm_loglik_grad_walk_refused", "hmm_loglik_grad_walk"}
    for name, (restype, argtypes) in engine.LOGLIK_GRAD_WALK_SIGNATURES.items():
        assert name not in engine._SIGNATURES and name not in engine.POSTERIOR_WALK_SIGNATURES
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes)


def test_wrappers_refuse(lib):
    for q in (16, 64, 257, 1027):
        with pytest.raises(ValueError, match="65..256"):
            engine.loglik_grad_walk(torch.eye(q)[None], torch.ones(q) / q, torch.rand(1, 2, 5, q))
        with pytest.raises(ValueError, match="65..256"):
            engine.loglik_grad_walk(torch.eye(q)[None], torch.ones(q) / q, torch.rand(1, 2, 5, q), want_grads=False)
    A, pi, E = torch.eye(71)[None], torch.ones(71) / 71, torch.rand(1, 2, 5, 71)
    with pytest.raises(engine.EngineError, match="HIP device"):                 # in range: there is no CPU path
        engine.loglik_grad_walk(A, pi, E)
    with pytest.raises(ValueError, match="support_only"):
        autograd.loglik(A, pi, E, support_only="yes")
    with pytest.raises(engine.EngineError, match="HIP device"):                 # "always" does not ask the predicate
        autograd.loglik(A, pi, E, support_only="always")
    assert GenePredMultiHMMTransitioner(k=5).support_grad is False
    tr = GenePredMultiHMMTransitioner(k=5, support_grad=True)
    assert tr.support_grad is True and GenePredMultiHMMTransitioner.from_config(tr.get_config()).support_grad is True


@pytest.mark.parametrize("spec", SPECS, ids=wc.spec_id)
def test_case_can_carry_the_gpu_comparison(spec):
    c = wc.build(spec)
    k, b, L, q = c["E"].shape
    assert (k, q, b, L) == (len(spec.models), spec.q, spec.b, spec.L)
    assert all(c[n].dtype == np.float32 for n in ("A", "pi", "E")) and c["A"].shape == (k, q, q) and c["pi"].shape == (k, q)
    assert wc.Q_MIN <= q <= wc.Q_MAX and k * b <= 130 and L <= 333               # every GPU case is small
    assert (c["w"] is None) == (spec.w == "none")
    if spec.w == "zeros":
        assert ((c["w"] == 0).sum(-1) == 3).all()
    if k == 2:
        assert not np.array_equal(c["A"][0], c["A"][1])
    assert wc.violations(spec) == []
    for m, ref in enumerate(wc.reference(spec)):
        A = c["A"][m]
        deg = np.maximum((A != 0).sum(0), (A != 0).sum(1))
        assert np.all(np.abs(A.astype(np.float64).sum(-1) - 1) < 1e-5) and np.all(A >= 0)
        if ref is None:
            assert spec.models[m] == wc.REFUSED and (deg > 8).sum() == 3         # outside the sparse rule
            continue
        copies = (q - 1) // 14
        assert (deg > 8).sum() == {"gene": int(copies + 1 > 8), "deg0": 0, "deg1": 1, "deg2": 2}[spec.models[m]]
        if spec.models[m] == "gene":
            assert deg[0] == copies + 1 and deg[1:].max() <= 8                  # the intergenic state: a hub from 8 copies
        assert set(ref["limit"]) == set(wc.FINE_NORMS)
        for n in wc.FINE_NORMS:
            assert ref["small"][n] <= 0.05 and 4 * ref["e32"][n] <= 1e-3, (m, n, ref["small"][n], ref["e32"][n])
            assert ref["limit"][n] == max(2e-4, 4 * ref["e32"][n])
        if L == 1:
            assert np.all(ref["want"][0] == 0.0)
        if spec.w == "zeros":
            assert np.all(ref["want"][2][c["w"][m] == 0] == 0.0)
        clampedE = c["E"][m] <= spec.eps
        assert np.all(ref["want"][2][clampedE] == 0.0) and np.all(ref["want"][1][c["pi"][m] <= spec.eps] == 0.0)
        if spec.emis == "mid" and spec.eps > wc.EPS:                            # clamped by the caller's eps alone
            assert (clampedE & (c["E"][m] > wc.EPS)).mean() > 0.1
        if spec.emis == "blank0":
            s = int(np.abs(c["w"][m]).argmax())
            assert np.all(c["E"][m, s, 0] == 0.0) and (c["E"][m, :, 0] == 0.0).all(-1).sum() == 1
        if spec.models[m] == "deg2":
            assert (c["pi"][m] <= spec.eps).sum() == 2


def test_the_sweep_covers_what_it_is_for():
    specs = wc.all_specs()
    assert len({wc.spec_id(s) for s in specs}) == len(specs)
    assert set(wc.SEEDS) <= {wc.spec_id(s) for s in specs + [wc.refused_case()]}          # no stale entry
    assert {(s.q, s.emis) for s in wc.gene_sweep()} == {(q, e) for q in (71, 127, 253) for e in ("holes", "rare", "dead")}
    assert any(s.L == 300 and s.q == q for s in wc.gene_sweep() for q in (71, 253))
    assert {(s.models[0], s.q) for s in wc.state_sweep()} == \
        {(kind, q) for kind in ("deg0", "deg1", "deg2") for q in (65, 96, 128, 129, 192, 193, 256)}
    assert {(s.q, s.L) for s in wc.length_sweep()} == {(q, L) for q in (71, 193) for L in (1, 2, 3, 7, 8, 9, 17, 300)}
    assert all(len(s.models) == 2 for s in wc.length_sweep())
    assert {(s.b, s.L) for s in wc.batch_sweep()} == {(b, 24) for b in (1, 3, 65, 130)}
    assert {s.emis for s in specs} == {"holes", "blank0", "dead", "mid", "rare"}
    assert {s.w for s in specs} == {"wide", "zeros", "none"} and {s.eps for s in specs} == {1e-16, 1e-6}
    assert any(s.w == "zeros" and s.b > 64 for s in specs)
    r = wc.refused_case()
    assert r.models == ("deg3", "deg1")


def test_build_is_deterministic_and_read_only():
    s = wc.weight_cases()[0]
    a = wc.build(s)
    wc._build.cache_clear()
    b = wc.build(s)
    assert a is not b and all(np.array_equal(a[n], b[n]) for n in a)
    with pytest.raises(ValueError):
        a["E"][0, 0, 0, 0] = 1.0


@pytest.mark.parametrize("seed", [0, 1])
def test_the_transitioner_never_reads_the_gradient_of_an_absent_edge(seed):
    """The mask proof: through make_A() of the five-copy transitioner, a random dense dA and the same dA with its
    off-support entries zeroed give bit-identical parameter gradients — probs = (softmax + 1e-16) * mask multiplies
    every off-support gradient by 0 before it can reach a parameter."""
    torch.manual_seed(seed)
    tr = GenePredMultiHMMTransitioner(k=5, initial_exon_len=200, initial_intron_len=4500, initial_ir_len=10000)
    A = tr.make_A()
    assert A.shape == (1, 71, 71)
    support = A.detach() != 0
    assert int(support.sum()) == 1 + 22 * 5
    dA = torch.randn(A.shape) * 10.0 ** torch.randint(-3, 4, A.shape).float()
    assert float(dA[~support].abs().min()) > 0
    dense = torch.autograd.grad(A, tr.transition_kernel, dA, retain_graph=True)[0]
    on_support = torch.autograd.grad(A, tr.transition_kernel, torch.where(support, dA, torch.zeros_like(dA)))[0]
    assert float(dense.abs().max()) > 0 and torch.equal(dense, on_support)
