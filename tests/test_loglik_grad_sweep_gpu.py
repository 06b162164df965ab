"""hmm_loglik_grad for 1..64 states on its four routes (scan16: csrc/hmm_grad.inc; wave: the one-wave-per-sequence
sweeps of csrc/hmm_midq.inc; pc29: pc_loglik_grad; gscan: hmm_loglik_grad_scan) against the fp64 oracle.  Needs an
MI355X.

Inputs, norms, limits and exclusions: tests/loglik_grad_cases.py (the tensor norms of tests/test_grad_gpu.py::check as
err / tolerance <= 1, and dA per row over present edges, dE per sequence and — on the wave route — dE per state column
at max(2e-4, 4 e32), e32 = the error of fp32 autograd through the restated reference loop on the CPU).
tests/test_loglik_grad_sweep_cpu.py shows from the oracle alone that the inputs can carry this.  Every test asserts
that its case took the route it is for.  Each comparison prints its figures (pytest -s) before it asserts.

Worst error / limit measured on an MI355X over all cases of this file, per route and norm (tensor norms: err is already
err / tolerance, and so is their e32), with the largest e32 of that route and norm.  The whole file takes 5 s.
    scan16 dA        0.006  (5.84e-03 of 1.00e+00, scan16-sparse-q1-b3-L203-rare-wide-c0 m=0);  e32 <= 1.5e-02 (scan16-dense-q1-b3-L203-holes-wide-c0)
    scan16 dA/absent 0.000  (1.75e-04 of 1.00e+00, scan16-shipped-q15-b7-L100-rare-wide-c16 m=0);  e32 <= 2.1e-04 (scan16-shipped-q15-b7-L100-rare-wide-c16)
    scan16 dpi       0.002  (1.66e-03 of 1.00e+00, scan16-gene+dense-q15-b3-L16-holes-wide-c0 m=1);  e32 <= 6.5e-03 (scan16-gene-q15-b3-L203-rare-wide-c0)
    scan16 dE        0.007  (7.32e-03 of 1.00e+00, scan16-gene-q7-b3-L203-rare-wide-c0 m=0);  e32 <= 3.4e-02 (scan16-gene-q15-b3-L203-rare-wide-c0)
    scan16 ll        0.005  (4.52e-03 of 1.00e+00, scan16-gene-q15-b3-L600-stretch-wide-c16 m=0);  e32 <= 8.5e-01 (scan16-sparse-q1-b3-L203-rare-wide-c0)
    scan16 dA/row    0.011  (2.29e-06 of 2.00e-04, scan16-shipped-q15-b7-L100-rare-wide-c16 m=0);  e32 <= 1.0e-04 (scan16-gene-q15-b3-L600-stretch-wide-c16)
    scan16 dE/seq    0.005  (1.03e-06 of 2.00e-04, scan16-gene-q7-b3-L203-rare-wide-c0 m=0);  e32 <= 1.4e-04 (scan16-gene-q15-b3-L600-stretch-wide-c16)
    wave   dA        0.006  (6.43e-03 of 1.00e+00, wave-sparse-q63-b3-L203-holes-wide-c0 m=0);  e32 <= 2.8e-03 (wave-dense-q32-b3-L203-holes-wide-c0)
    wave   dA/absent 0.000  (2.61e-04 of 1.00e+00, wave-sparse-q63-b3-L203-holes-wide-c0 m=0);  e32 <= 3.2e-04 (wave-gene-q43-b3-L203-dead-wide-c0)
    wave   dpi       0.003  (3.11e-03 of 1.00e+00, wave-dense+sparse-q32-b3-L17-holes-wide-c0 m=1);  e32 <= 5.0e-03 (wave-gene-q57-b3-L203-dead-wide-c0)
    wave   dE        0.003  (3.35e-03 of 1.00e+00, wave-dense+sparse-q32-b3-L16-holes-wide-c0 m=1);  e32 <= 2.7e-02 (wave-gene-q57-b3-L203-rare-wide-c0)
    wave   ll        0.035  (3.53e-02 of 1.00e+00, wave-gene-q29-b3-L203-dead-wide-c0 m=0);  e32 <= 2.8e-01 (wave-gene-q43-b3-L203-dead-wide-c0)
    wave   dA/row    0.198  (3.97e-05 of 2.00e-04, wave-gene+sparse-q43-b130-L24-holes-wide-c0 m=0);  e32 <= 7.5e-05 (wave-gene-q57-b3-L203-holes-wide-c0)
    wave   dE/seq    0.003  (6.10e-07 of 2.00e-04, wave-gene-q43-b3-L203-holes-wide-c0 m=0);  e32 <= 1.2e-06 (wave-gene-q57-b3-L203-holes-wide-c0)
    wave   dE/col    0.006  (1.30e-06 of 2.00e-04, wave-gene-q29-b3-L203-rare-wide-c0 m=0);  e32 <= 1.7e-04 (wave-gene-q57-b3-L203-holes-wide-c0)
    pc29   dA        0.000  (2.64e-04 of 1.00e+00, pc29-gene-q29-b5-L97-holes-wide-c16 m=0);  e32 <= 1.7e-03 (pc29-gene-q29-b3-L333-holes-wide-c16)
    pc29   dA/absent 0.000  (2.19e-04 of 1.00e+00, pc29-gene-q29-b2-L700-holes-wide-c0 m=0);  e32 <= 8.7e-04 (pc29-gene-q29-b2-L700-holes-wide-c0)
    pc29   dpi       0.001  (9.84e-04 of 1.00e+00, pc29-gene-q29-b3-L333-holes-wide-c16 m=0);  e32 <= 2.8e-03 (pc29-gene-q29-b2-L700-holes-wide-c0)
    pc29   dE        0.005  (5.15e-03 of 1.00e+00, pc29-gene-q29-b3-L333-holes-wide-c16 m=0);  e32 <= 2.6e-02 (pc29-gene-q29-b5-L97-holes-wide-c16)
    pc29   ll        0.004  (3.58e-03 of 1.00e+00, pc29-gene-q29-b3-L333-holes-wide-c16 m=0);  e32 <= 5.4e-01 (pc29-gene-q29-b2-L700-holes-wide-c0)
    pc29   dA/row    0.026  (5.15e-06 of 2.00e-04, pc29-gene-q29-b2-L700-holes-wide-c0 m=0);  e32 <= 1.6e-05 (pc29-gene-q29-b2-L700-holes-wide-c0)
    pc29   dE/seq    0.002  (4.87e-07 of 2.00e-04, pc29-gene-q29-b3-L97-blank0-wide-c16 m=0);  e32 <= 6.0e-07 (pc29-gene-q29-b2-L700-holes-wide-c0)
    gscan  dA        0.001  (7.20e-04 of 1.00e+00, gscan-dense-q49-b3-L203-holes-wide-c16 m=0);  e32 <= 2.8e-03 (gscan-dense-q32-b3-L203-holes-wide-c16)
    gscan  dA/absent 0.000  (7.94e-05 of 1.00e+00, gscan-gene-q43-b3-L203-holes-wide-c16 m=0);  e32 <= 1.0e-04 (gscan-gene-q43-b3-L203-holes-wide-c16)
    gscan  dpi       0.001  (1.42e-03 of 1.00e+00, gscan-gene-q43-b3-L203-holes-wide-c16 m=0);  e32 <= 2.5e-03 (gscan-gene-q57-b3-L203-holes-wide-c16)
    gscan  dE        0.004  (3.60e-03 of 1.00e+00, gscan-gene-q57-b3-L203-holes-wide-c16 m=0);  e32 <= 1.3e-02 (gscan-gene-q57-b3-L203-holes-wide-c16)
    gscan  ll        0.006  (5.55e-03 of 1.00e+00, gscan-dense-q49-b3-L203-holes-wide-c16 m=0);  e32 <= 1.8e-01 (gscan-dense-q32-b3-L203-holes-wide-c16)
    gscan  dA/row    0.003  (1.01e-06 of 3.02e-04, gscan-gene-q57-b3-L203-holes-wide-c16 m=0);  e32 <= 7.5e-05 (gscan-gene-q57-b3-L203-holes-wide-c16)
    gscan  dE/seq    0.002  (3.44e-07 of 2.00e-04, gscan-gene-q57-b3-L203-holes-wide-c16 m=0);  e32 <= 1.2e-06 (gscan-gene-q57-b3-L203-holes-wide-c16)
With the routing off (EXACT_OFF) the window case's flagged sequence has dE/seq 3.4e-2 against its limit of 5.7e-4.

What the sweep found: dpi lost w gamma_0[j] of every sequence whose first emission of state j is clamped (it was read
off dE's first row, where clamped entries are 0).  That is negligible unless the whole first row is clamped or q = 1,
where it is the entire gradient: dpi err / tolerance 5000 (100 % of max|dpi|) on scan16 q = 1 with holes and on the
three blank0 cases before the fix, <= 3e-3 after it.
"""
import contextlib

import numpy as np
import pytest
import torch

from hmm_layer_amd import engine

import loglik_grad_cases as lc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(x):
    return torch.as_tensor(np.array(x, dtype=np.float32, order="C"), device=DEV)    # (a copy: the cases are read-only)


def run(spec, A, pi, E, w, routed=None):
    """numpy (k,q,q), (k,q), (k,b,L,q), (k,b) | None -> numpy dA, dpi, dE, ll on the spec's route, which is asserted.
    routed: for scan16, what exact_detail must say — "none" (default for primitive models), "model" (default for the
    others: the model check sends every sequence to the serial plan), "windows", or "any" (no assertion)."""
    dims = tuple(E.shape)
    k, b, L, q = dims
    args = (dev(A), dev(pi), dev(E), None if w is None else dev(w))
    with contextlib.ExitStack() as st:
        st.enter_context(engine.option(engine.OPT_CHUNK, spec.chunk))
        if spec.route == "scan16":
            assert q <= 16
            out = engine.loglik_grad(*args)
            det = engine.exact_detail(dims)
            routed = routed or ("none" if lc.primitive(spec) else "model")
            if routed == "none":
                assert det["routed"] == 0, det
            elif routed == "model":
                assert det["routed"] == k * b and det["window_sequences"] == 0 and det["whole"] == 0, det
            elif routed == "windows":
                assert det["windows"] >= 1 and det["whole"] == 0, det
        elif spec.route == "wave":
            st.enter_context(engine.option(engine.OPT_PGCHUNK, 0))
            out = engine.loglik_grad(*args)
            assert 16 < q <= 64 and engine.loglik_grad_serial_count(dims) == k * b
        elif spec.route == "pc29":
            st.enter_context(engine.option(engine.OPT_PGCHUNK, 2))
            out = engine.loglik_grad(*args)
            assert engine.loglik_grad_serial_count(dims) == 0
        elif spec.route == "gscan":
            out = engine.loglik_grad_scan(*args)
            assert L > engine.lib().hmm_loglik_grad_scan_chunk_len(*dims)               # at least two chunks
            assert engine.loglik_grad_scan_serial_count(dims) == 0
        else:
            raise ValueError(spec.route)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def run_case(spec, routed=None):
    c = lc.build(spec)
    return run(spec, c["A"], c["pi"], c["E"], c["w"], routed)


def check(spec, got=None, routed=None):
    """The case on the engine against the oracle under every norm -> (inputs, [dA, dpi, dE, ll], reference)."""
    c = lc.build(spec)
    ref = lc.reference(spec)
    got = got or run_case(spec, routed)
    failed = []
    for m, r in enumerate(ref):
        mine = [x[m] for x in got]
        assert all(np.isfinite(x).all() for x in mine), (lc.spec_id(spec), m)
        err, _ = lc.errors(mine, r, c["A"][m], spec.route)
        for norm, lim in lc.limits(r).items():
            print("LLSWEEP %s m=%d %s err %.3e limit %.3e e32 %.3e" % (lc.spec_id(spec), m, norm, err[norm], lim, r["e32"][norm]))
            if not err[norm] <= lim:
                failed.append((m, norm, err[norm], lim))
        assert np.all(mine[2][c["E"][m] <= lc.EPS] == 0.0), (lc.spec_id(spec), m)     # clamped emissions: exactly 0
        assert np.all(mine[1][c["pi"][m] <= lc.EPS] == 0.0), (lc.spec_id(spec), m)    # clamped pi entries: exactly 0
    assert not failed, (lc.spec_id(spec), failed)
    return c, got, ref


@pytest.mark.parametrize("spec", lc.state_sweep(), ids=lc.spec_id)
def test_state_sweep(spec):
    """wave: q at both ends of and inside every QB block and the 29-, 43- and 57-state gene models; scan16: every
    register group of the 16-state tile and the 7- and 15-state gene topologies.  L = 203 = 25 prefetch blocks of 8 and
    a tail of 3; holes / rare / dead emissions; weights +-10^U(-3,3)."""
    c, got, _ = check(spec)
    if spec.emis in ("holes", "dead"):
        assert (c["E"] <= lc.EPS).any()


@pytest.mark.parametrize("spec", lc.length_sweep(), ids=lc.spec_id)
def test_length_sweep_two_models(spec):
    """L around one and two prefetch blocks, two different models in one call."""
    c, got, _ = check(spec)
    if spec.L == 1:
        assert np.all(got[0] == 0.0)


@pytest.mark.parametrize("spec", lc.batch_sweep(), ids=lc.spec_id)
def test_batch_sweep_and_each_sequence_alone(spec):
    """b on both sides of the 64-lane stride of k_mq_grad_sum / k_mq_grad_pi / k_grad_pi, two models; on the wave
    route a sequence's dE is that of the sequence run alone, bit for bit (one wave per sequence, nothing shared)."""
    c, got, _ = check(spec)
    if spec.route == "wave":
        for s in range(spec.b):
            alone = run(spec, c["A"], c["pi"], c["E"][:, s:s + 1], c["w"][:, s:s + 1])
            assert np.array_equal(alone[2][:, 0], got[2][:, s]), s


@pytest.mark.parametrize("spec", lc.weight_cases(), ids=lc.spec_id)
def test_weights_and_initial_distribution(spec):
    """Sequences of weight 0 (their dE rows exactly 0, nothing NaN), no weights at all, pi entries below eps (their dpi
    exactly 0), a model with states nothing enters, a sequence whose whole first row is clamped (dpi keeps its
    gamma_0; on scan16 such a sequence may be routed)."""
    c, got, _ = check(spec, routed="any" if spec.emis == "blank0" else None)
    if spec.w == "zeros":
        zero = c["w"] == 0.0
        assert zero.sum() == 3 * len(spec.models) and np.all(got[2][zero] == 0.0)
    if "tinypi" in spec.models or "deadin" in spec.models:
        tiny = c["pi"] <= lc.EPS
        assert tiny.sum() == 2 and np.all(got[1][tiny] == 0.0)


@pytest.mark.parametrize("spec", lc.clamp_cases(), ids=lc.spec_id)
def test_clamped_forward_recursion(spec):
    """The `live` sign bit of k_mq_backward_grad at every t >= 1, q = 40 (QB 48) and q = 60 (QB 64); the 1e-20 edge
    into the clamped state keeps what the backward recursion sends it."""
    c, got, ref = check(spec)
    D, rA = spec.q - 1, ref[0]["want"][0]
    assert c["A"][0, 0, D] > 0
    assert abs(got[0][0, 0, D] - rA[0, D]) <= 2e-4 * np.abs(rA).max()


def test_window_case_and_what_the_windows_repair():
    """scan16 with HMM_OPT_CHUNK = 16: one sequence carries a four-position stretch that only a leave-after-one-step
    state can emit; it is flagged and recomputed in windows (none whole).  With the routing off its dE misses the
    finer dE/seq limit: the input bites."""
    spec = lc.window_case()
    c, got, ref = check(spec, routed="windows")
    with engine.option(engine.OPT_EXACT, engine.EXACT_OFF):
        off = run_case(spec, routed="any")
    s, wE = lc.STRETCH_SEQ, ref[0]["want"][2]
    err = np.abs(off[2][0, s] - wE[s]).max() / np.abs(wE[s]).max()
    print("LLSWEEP %s EXACT_OFF dE/seq of sequence %d: %.3e limit %.3e" % (lc.spec_id(spec), s, err, ref[0]["limit"]["dE/seq"]))
    assert err > ref[0]["limit"]["dE/seq"]


def test_reducible_model_goes_whole_to_the_serial_plan():
    check(lc.shipped_case(), routed="model")


@pytest.mark.parametrize("spec", lc.pc29_cases(), ids=lc.spec_id)
def test_compiled_29_state_topology_per_chunk(spec):
    check(spec)


@pytest.mark.parametrize("spec", lc.gscan_cases(), ids=lc.spec_id)
def test_loglik_grad_scan_on_the_wave_inputs(spec):
    """13 chunks of 16 positions, the last one ragged; both row widths."""
    c, got, _ = check(spec)
    wave = [s for s in lc.wave_state_sweep() if lc.build(s) is c]
    assert len(wave) == 1                                    # the same arrays as the wave case


ROUTE_PAIRS = {"wave": ("wave-gene+dense-q43-b3-L9", "wave-gene+sparse-q43-b130-L24"),
               "scan16": ("scan16-gene+dense-q15-b3-L9", "scan16-gene+sparse-q15-b130-L24"),
               "pc29": ("pc29-gene-q29-b5-L97", "pc29-gene-q29-b2-L700"),
               "gscan": ("gscan-dense-q17-b3-L203", "gscan-gene-q57-b3-L203")}


def _named(prefix):
    hit = [s for s in lc.all_specs() if lc.spec_id(s).startswith(prefix + "-")]
    assert len(hit) == 1, prefix
    return hit[0]


@pytest.mark.parametrize("route", lc.ROUTES)
def test_deterministic_and_workspace_reuse(route):
    """Two calls give identical bits; the engine keeps its workspace between calls: a small case, a larger one (the
    workspace grows), the small one again — identical bits."""
    X, Y = (_named(p) for p in ROUTE_PAIRS[route])
    engine.release_workspaces()
    first = run_case(X)
    second = run_case(X)
    check(Y)
    again = run_case(X)
    for a, b, c in zip(first, second, again):
        assert np.array_equal(a, b) and np.array_equal(a, c)
    check(X, again)
