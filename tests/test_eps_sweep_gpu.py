"""The caller's clamp eps through hmm_forward, hmm_backward, hmm_posterior (three modes), hmm_posterior_decode /
_decode_mid, hmm_posterior_grad and hmm_posterior_grad_scan for 1..64 states, against the fp64 oracle at that eps.
Needs an MI355X.

Cases, references and limits: tests/eps_cases.py; tests/test_eps_sweep_cpu.py shows from the oracle alone that every
case moves by at least ten tolerances between eps = 1e-16 and its own eps, so a kernel that assumed the default
anywhere — the emission floor of the chunk operators, k_topo_check's support test, the certificates, the denormal-range
marks, the clamp flags of the gradient sweeps — misses by that much.  Tolerances are those of tests/test_engine_gpu.py:
gamma 2e-5, log-likelihood 1e-6 |ll| + 2e-4, log alpha / log beta through assert_log_close_in_probability_space
(POST_LOG_NO_LL: 2e-5 + 2.4e-7 max |ll| after the log-likelihood is taken out, tests/test_exact_gpu.py).  The pure
log-space checks of that file would apply where the oracle's value exceeds max(1e-4, 1e12 eps) (its masks, g64 > 1e-4
and x64 > -30, assume clamp-only values near 1e-16).  That bound is at least 1 for every eps of the table (100 at
1e-10), so none of them runs here, which the test asserts and prints; log gamma, log alpha and log beta are compared as
probabilities.  The gradients use the norms and limits of tests/postgrad_mid_cases.py / postgrad_small_cases.py.  Every
comparison prints its figures (pytest -s) before it asserts.

Measured on an MI355X (every figure below is printed by the tests; error / limit, with the case):
    at HMM_EPS_MIN: gamma  0.416  (3.664e-05 of 8.802e-05, gene-q15-b3-L200-blank-eps1e-18-T16, gamma/log+ll)
    at HMM_EPS_MIN: loglik             0.031  (3.062e-02 of 1.000e+00, gene-q29-b2-L641-blank-eps1e-18-T16, loglik/prob)
    at HMM_EPS_MIN: posterior_grad     0.004  (1.097e-06 of 3.000e-04, gene-q15-b3-L200-blank-eps1e-18-T16, chunk, prob)
    at HMM_EPS_MIN: posterior_grad_scan 0.003  (8.385e-07 of 3.000e-04, gene-q29-b2-L641-blank-eps1e-18-T16, log)
    conf                               0.007  (1.318e-07 of 2.000e-05, dense-q2-b3-L200-rare-eps1e-06-T16)
    gamma                              0.607  (1.663e-04 of 2.739e-04, gene-q15-b2-L641-rare-eps1e-10, gamma/log+ll)
    loglik                             0.036  (3.581e-02 of 1.000e+00, gene-q29-b3-L641-rare-eps1e-10-T16, loglik/prob)
    posterior_grad dE/col  0.161  (4.845e-05 of 3.000e-04, gene-q29-b3-L203-rare-eps1e-06-prob-whole; e32 5.643e-05)
    posterior_grad dE/seq  0.033  (9.926e-06 of 3.000e-04, gene-q7-b3-L100-zeros-eps1e-06-T16-prob-chunk; e32 7.452e-06)
    posterior_grad dA/row  0.113  (3.393e-05 of 3.000e-04, gene-q57-b2-L60-edge-eps1e-06-prob-whole; e32 4.255e-05)
    posterior_grad tensor  0.009  (2.762e-06 of 3.000e-04, gene-q29-b3-L203-rare-eps1e-06-prob-whole; e32 9.212e-07)
    posterior_grad dA/absent           9.2e-07 of the largest entry of dA (gene-q7-b3-L100-zeros-eps1e-06-T16-log-chunk)
No case needed the conditioning rule: eps_cases.CONDITIONED is empty, every limit above is the stated tolerance.

Routes of engine.posterior at the case's eps (test_every_route_is_taken_at_a_non_default_eps; sequences that left
the scan / sequences of the call):
    gene-q15-b3-L200-plain-eps1e-06-T16          whole    3 / 3
    gene-q15-b3-L200-plain-eps0.001-T16          model    3 / 3
    gene-q15-b3-L200-rare-eps1e-10-T16           whole    3 / 3
    gene-q15-b3-L200-zeros-eps1e-06-T16          whole    3 / 3
    gene-q15-b2-L641-blank-eps1e-06-T16          whole    2 / 2
    gene-q15-b3-L200-edge-eps1e-06-T16           whole    3 / 3
    gene-q15-b2-L1-blank-eps1e-10-T16            scan     0 / 2
    gene-q15-b5-L17-rare-eps0.001-T16            model    5 / 5
    gene-q15-b2-L641-rare-eps1e-10               whole    2 / 2
    gene-q7-b3-L200-rare-eps1e-06-T16            whole    3 / 3
    gene-q7-b4-L17-zeros-eps0.001-T16            model    4 / 4
    gene-q7-b2-L641-blank-eps1e-10-T16           scan     0 / 2
    gene-q7-b2-L641-blank-eps1e-06-T16           windows  1 / 2, 1 windows over 37 chunks
    gene-q7-b2-L961-blank-eps1e-06-T16           windows  2 / 2, 5 windows over 63 chunks
    gene-fd-q15-b3-L200-rare-eps1e-06-T16        whole    3 / 3
    gene-fd-q15-b2-L641-blank-eps0.001-T16       model    2 / 2
    dense-q1-b5-L17-rare-eps1e-06-T16            scan     0 / 5
    dense-q2-b3-L200-rare-eps1e-06-T16           scan     0 / 3
    dense-q5-b3-L200-rare-eps0.001-T16           scan     0 / 3
    dense-q5-b2-L1-blank-eps1e-06-T16            scan     0 / 2
    dense-q13-b3-L200-edge-eps0.001-T16          scan     0 / 3
    dense-q16-b2-L641-rare-eps0.001-T16          scan     0 / 2
    dense-q16-b2-L641-blank-eps1e-06-T16         scan     0 / 2
    dense-q13-b2-L641-blank-eps1e-10-T16         scan     0 / 2
    triu-q7-b3-L200-rare-eps0.001-T16            model    3 / 3
    thin-q7-b3-L200-plain-eps0.001-T16           model    3 / 3
    thin-q16-b2-L200-plain-eps0.001-T16          model    2 / 2
    dense+triu-q7-b2-L200-rare-eps0.001-T16      model    2 / 4
    gene-q29-b3-L641-rare-eps1e-10-T16           whole    3 / 3
    gene-q29-b3-L203-plain-eps1e-06              whole    3 / 3
    gene-q29-b2-L641-blank-eps1e-06-T16          whole    2 / 2
    gene-q29-b4-L17-zeros-eps0.001-T16           model    4 / 4
    gene-q43-b2-L641-rare-eps1e-06-T16           whole    2 / 2
    gene-q43-b3-L17-edge-eps1e-06-T16            walk     0 / 3
    gene-q57-b3-L100-zeros-eps1e-06-T16          walk     0 / 3
    gene-q57-b1-L641-blank-eps1e-10-T16          scan     0 / 1
    dense-q17-b3-L200-rare-eps0.001-T16          scan     0 / 3
    dense-q32-b2-L641-rare-eps0.001-T16          scan     0 / 2
    dense-q33-b2-L641-rare-eps0.001-T16          scan     0 / 2
    dense-q48-b3-L100-blank-eps1e-06-T16         walk     0 / 3
    dense-q64-b5-L17-rare-eps0.001-T16           walk     0 / 5
    dense-q64-b1-L641-zeros-eps0.001-T16         scan     0 / 1
    dense-q64-b2-L1-blank-eps1e-06-T16           walk     0 / 2
    triu-q20-b2-L641-rare-eps0.001-T16           model    2 / 2
    thin-q24-b2-L641-plain-eps0.001-T16          model    2 / 2
    dense+triu-q20-b2-L641-rare-eps0.001-T16     model    2 / 4
Counts: up to 16 states whole 8, model 8, scan 10, windows 2; 17..64 states whole 4, model 4, walk 5, scan 5.
    thin-q7-b3-L200-plain-eps0.001-T16: scan at 1e-16, model at its eps (the support changes)
    thin-q16-b2-L200-plain-eps0.001-T16: scan at 1e-16, model at its eps (the support changes)
    thin-q24-b2-L641-plain-eps0.001-T16: scan at 1e-16, model at its eps (the support changes)

    handover (gene-q7-b2-L961-blank-eps1e-06-T16, sequence 1): windows [(0, 14), (15, 13), (29, 12)], psi[14] 6.364e-05,
        err 3.078e-07; unrouted 5.080e-05
    handover q=12 mode 0: 1 sequence left the scan, err 5.914e-08
    handover q=12 mode 1: 1 sequence left the scan, err 1.686e-07
    handover q=12 mode 2: 1 sequence left the scan, err 9.251e-06
    handover q=12: unrouted err 2.549e-04
    handover q=24 mode 0: 1 sequence left the scan, err 3.964e-08
    handover q=24 mode 1: 1 sequence left the scan, err 1.442e-07
    handover q=24 mode 2: 1 sequence left the scan, err 6.045e-06
    handover q=24: unrouted err 2.472e-03
    handover q=48 mode 0: 1 sequence left the scan, err 1.699e-08
    handover q=48 mode 1: 1 sequence left the scan, err 6.766e-08
    handover q=48 mode 2: 1 sequence left the scan, err 2.923e-06
    handover q=48: unrouted err 7.101e-04
    layer: gamma err 1.544e-06 (limit 2e-5; the oracle moves by 9.973e-01 from eps = 1e-16)

Sequences of the gradient cases that the whole-sequence sweeps served.  All of them, under HMM_OPT_PGCHUNK = 1 as well: the
floor-transition certificate F = eps sum_t 1 / Sg_t is at least eps L, above its threshold of 2e-6 for every case of
eps >= 1e-6, and the rare emissions of the 1e-10 case make Sg small enough.  What these cases hold of the per-chunk
evaluation and of hmm_posterior_grad_scan at a non-default eps is therefore that verdict and the values of the
sweeps it hands over to; the per-chunk sums themselves stay covered at the default eps only
(tests/test_postgrad_small_gpu.py, tests/test_posterior_grad_scan_gpu.py):
    gene-q15-b3-L200-rare-eps1e-06-T16-prob-chunk        3 of 3
    gene-q15-b3-L200-rare-eps1e-06-T16-log-chunk         3 of 3
    gene-q15-b3-L200-edge-eps1e-10-T16-prob-chunk        3 of 3
    gene-q15-b3-L200-edge-eps1e-10-T16-log-chunk         3 of 3
    dense-q5-b3-L200-edge-eps0.001-T16-prob-chunk        3 of 3
    dense-q5-b3-L200-edge-eps0.001-T16-log-chunk         3 of 3
    gene-q7-b3-L100-zeros-eps1e-06-T16-prob-chunk        3 of 3
    gene-q7-b3-L100-zeros-eps1e-06-T16-log-chunk         3 of 3
    dense-q16-b3-L203-edge-eps0.001-T16-prob-chunk       3 of 3
    dense-q16-b3-L203-edge-eps0.001-T16-log-chunk        3 of 3
    thin-q7-b3-L200-plain-eps0.001-T16-prob-chunk        3 of 3
    thin-q7-b3-L200-plain-eps0.001-T16-log-chunk         3 of 3
    dense-q2-b3-L17-edge-eps1e-06-T16-prob-chunk         3 of 3
    dense-q2-b3-L17-edge-eps1e-06-T16-log-chunk          3 of 3
    gene-q29-b2-L641-edge-eps1e-06-T16-prob-scan         2 of 2
    gene-q29-b2-L641-edge-eps1e-06-T16-log-scan          2 of 2
    gene-q43-b2-L641-rare-eps1e-06-T16-prob-scan         2 of 2
    gene-q43-b2-L641-rare-eps1e-06-T16-log-scan          2 of 2
"""
import contextlib

import numpy as np
import pytest
import torch

import eps_cases as ec
import postgrad_mid_cases as pm
import postgrad_small_cases as ps
import posterior_decode_ref as dref
from hmm_layer_amd import engine
from test_engine_gpu import assert_log_close_in_probability_space

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODES = (engine.POST_PROB, engine.POST_LOG, engine.POST_LOG_NO_LL)


def dev(x):
    return torch.as_tensor(np.array(x, dtype=np.float32, order="C"), device=DEV)    # (a copy: the cases are read-only)


@contextlib.contextmanager
def options(spec):
    with engine.option(engine.OPT_CHUNK, spec.T), \
            engine.option(engine.OPT_FORCE_DENSE, int("gene-fd" in spec.models)):
        yield


def primitive(A, eps):
    """k_topo_check on the host: the support of A (entries > eps) has a positive power (2^13 steps cover 64 states)."""
    B = np.asarray(A) > eps
    for _ in range(13):
        B = (B.astype(np.int64) @ B.astype(np.int64)) > 0
    return bool(B.all())


def route(spec, eps):
    """engine.posterior(POST_PROB) on the case at `eps` -> (the route's name, its counters, gamma, loglik).
    Up to 16 states: "scan" (no sequence left it), "model" (only the sequences of non-primitive models did), "windows" /
    "whole" (the certificates sent sequences of a primitive model to windows / to the whole-sequence kernel; a case with
    both counts as "windows").  17..64 states: "scan", "model", "whole" by the count of the one-wave kernels; "walk"
    where the shape plans no chunked scan at all."""
    c = ec.build(spec)
    dims = c["E"].shape
    e = ec.eps32(eps)
    with options(spec):
        out, ll = engine.posterior(dev(c["A"]), dev(c["pi"]), dev(c["E"]), eps=e)
        n = engine.exact_count(engine.OP_POSTERIOR, dims)
        det = engine.exact_detail(dims) if spec.q <= 16 else dict(routed=n)
        chunked = spec.q <= 32 or (engine.lib().hmm_workspace_bytes(engine.OP_POSTERIOR, *dims)
                                   > engine.lib().hmm_workspace_bytes(engine.OP_LOGLIK, *dims))
    by_model = spec.b * sum(not primitive(c["A"][m], e) for m in range(dims[0]))
    if not chunked:
        name = "walk"
    elif n == 0:
        name = "scan"
    elif n == by_model:
        name = "model"
    elif spec.q <= 16 and det["window_sequences"] > 0:
        name = "windows"
    else:
        name = "whole"
    return name, det, out.cpu().numpy(), ll.cpu().numpy()


def report(tag, spec, what, err, tol):
    print("EPS %s %s %s err %.3e limit %.3e (%.3f)" % (tag, ec.spec_id(spec), what, err, tol, err / tol))
    return err <= tol


@pytest.mark.parametrize("spec", ec.posterior_cases(), ids=ec.spec_id)
def test_posterior_forward_backward_at_the_callers_eps(spec):
    c, ref, e = ec.build(spec), ec.reference(spec), ec.eps32(spec.eps)
    A, pi, E = dev(c["A"]), dev(c["pi"]), dev(c["E"])
    dims = c["E"].shape
    lg_gamma, lg_ll = ec.limit(spec, "gamma"), ec.limit(spec, "ll")
    assert max(1e-4, 1e12 * e) >= 1.0                        # pure log space: only where the oracle's value exceeds this
    print("EPS %s: eps = %g leaves no value for the pure log-space checks" % (ec.spec_id(spec), spec.eps))
    failed = []
    with options(spec):
        outs = {}
        for mode in MODES:
            out, ll = engine.posterior(A, pi, E, mode=mode, eps=e)
            outs[mode] = (out.cpu().numpy(), ll.cpu().numpy())
        n = engine.exact_count(engine.OP_POSTERIOR, dims)
        print("EPS route %s: %d of %d sequences left the scan%s" % (
            ec.spec_id(spec), n, dims[0] * dims[1], " " + str(engine.exact_detail(dims)) if spec.q <= 16 else ""))
        la, ll_f = engine.forward(A, pi, E, eps=e)
        _, ll_l = engine.forward(A, pi, E, want_log_alpha=False, eps=e)
        lb = engine.backward(A, E, eps=e)
        la, ll_f, ll_l, lb = la.cpu().numpy(), ll_f.cpu().numpy(), ll_l.cpu().numpy(), lb.cpu().numpy()
        label, conf, ll_d = engine.posterior_decode(A, pi, E, eps=e)
    for m, r in enumerate(ref):
        tag = "m=%d" % m
        g64, ll64 = r["gamma"], r["ll"]
        tol_ll = ec.tol_loglik(ll64) * lg_ll
        for mode, name in zip(MODES, ("prob", "log", "log+ll")):
            got, ll = outs[mode][0][m], outs[mode][1][m]
            assert np.isfinite(ll).all(), (ec.spec_id(spec), name)
            tol = ec.TOL_GAMMA * lg_gamma
            if mode == engine.POST_LOG_NO_LL:
                got = got - ll[:, None, None]
                tol += 2.4e-7 * np.abs(ll64).max()
            p = got if mode == engine.POST_PROB else np.exp(got)
            assert np.isfinite(p).all(), (ec.spec_id(spec), name)
            if not report(tag, spec, "gamma/" + name, float(np.abs(p - g64).max()), tol):
                failed.append(("gamma", name, m))
            if not report(tag, spec, "loglik/" + name, float((np.abs(ll - ll64) / tol_ll).max()), 1.0):
                failed.append(("loglik", name, m))
        for name, ll in (("forward", ll_f[m]), ("loglik-only", ll_l[m])):
            if not report(tag, spec, "loglik/" + name, float((np.abs(ll - ll64) / tol_ll).max()), 1.0):
                failed.append(("loglik", name, m))
        for name, x, x64 in (("log alpha", la[m], r["la"]), ("log beta", lb[m], r["lb"])):
            assert not np.isnan(x).any(), (ec.spec_id(spec), name)
            assert_log_close_in_probability_space(x, x64, (ec.spec_id(spec), name, m))
    # decoding with the identity map: the decode kernels share every instruction up to the gamma row
    gamma, ll = outs[engine.POST_PROB]
    assert np.array_equal(label.cpu().numpy(), gamma.argmax(-1).astype(np.uint8)), ec.spec_id(spec)
    assert np.array_equal(conf.cpu().numpy(), gamma.max(-1)), ec.spec_id(spec)
    assert np.array_equal(ll_d.cpu().numpy(), ll), ec.spec_id(spec)
    assert not failed, (ec.spec_id(spec), failed)


def test_every_route_is_taken_at_a_non_default_eps():
    """Over the table, at the cases' own eps: up to 16 states the scan alone, windows, the whole-sequence kernel and
    the per-model route; for 17..64 the scan alone, sequences redone whole, the per-model route, and shapes that plan
    no chunked scan at all (the one-wave walk).  A call of two models mixes a scan-served and a routed one."""
    seen = {False: {}, True: {}}
    for spec in ec.posterior_cases():
        name, det, _, _ = route(spec, spec.eps)
        print("EPS route %s: %s %s" % (ec.spec_id(spec), name, det))
        seen[ec.is_mid(spec)].setdefault(name, []).append(ec.spec_id(spec))
        if len(spec.models) == 2:                            # (dense, triu): the dense model's sequences stay in the scan,
            assert name == "model" and det["routed"] == spec.b, (ec.spec_id(spec), name, det)    # the other's are routed
    assert {"scan", "windows", "whole", "model"} <= set(seen[False]), seen[False]
    assert {"scan", "whole", "model", "walk"} <= set(seen[True]), seen[True]


def test_a_clamp_between_two_chunks_is_certified():
    """eps_cases.HANDOVER: the only reverse clamp of its second sequence acts on the vector that chunk 14 hands to
    chunk 13.  The sequence leaves the scan (its certificate sum, charged to chunk 14, exceeds EXACT_DELTA) and meets
    the oracle; with the routing off the scan's values are off by 5e-5 before the clamp."""
    s = ec.HANDOVER
    c, r, e = ec.build(s), ec.reference(s)[0], ec.eps32(s.eps)
    seq, t = ec.HANDOVER_AT
    name, det, g, _ = route(s, s.eps)
    with options(s):
        wt = engine.window_table(c["E"].shape, seq)
        with engine.option(engine.OPT_EXACT, engine.EXACT_OFF):
            off, _ = engine.posterior(dev(c["A"]), dev(c["pi"]), dev(c["E"]), eps=e)
    err, err_off = np.abs(g[0, seq] - r["gamma"][seq]).max(), np.abs(off.cpu().numpy()[0, seq] - r["gamma"][seq]).max()
    print("EPS handover: %s %s windows %s psi[%d] %.3e err %.3e, unrouted %.3e" % (
        name, det, wt["windows"], t // s.T + 1, wt["psi"][t // s.T + 1], err, err_off))
    assert wt["psi"][t // s.T + 1] > 2e-6 and wt["windows"]
    assert err <= ec.TOL_GAMMA < err_off


@pytest.mark.parametrize("q", ec.HANDOVER_Q)
def test_a_clamp_between_two_chunks_is_certified_at_every_row_width(q):
    """eps_cases.handover_case for the 16-state rows, the 32-lane and the 64-lane rows of the chunked scan: the only
    clamp of the sequence acts on the vector one chunk hands to the one before.  The sequence leaves the scan and
    meets the oracle in all three modes and in the fused decode; with the routing off the scan misses."""
    from oracle import textbook
    c, e = ec.handover_case(q), ec.eps32(ec.HANDOVER_EPS)
    A, pi, E = dev(c["A"]), dev(c["pi"]), dev(c["E"])
    dims = c["E"].shape
    g64, ll64 = textbook.posterior(c["A"][0], c["pi"][0], c["E"][0], eps=e)
    with engine.option(engine.OPT_CHUNK, ec.HANDOVER_T):
        assert q <= 32 or (engine.lib().hmm_workspace_bytes(engine.OP_POSTERIOR, *dims)
                           > engine.lib().hmm_workspace_bytes(engine.OP_LOGLIK, *dims))     # the chunked scan is planned
        for mode in MODES:
            out, ll = engine.posterior(A, pi, E, mode=mode, eps=e)
            n = engine.exact_count(engine.OP_POSTERIOR, dims)
            got, ll = out.cpu().numpy()[0], ll.cpu().numpy()[0]
            if mode == engine.POST_LOG_NO_LL:
                got = got - ll[:, None, None]
            p = got if mode == engine.POST_PROB else np.exp(got)
            err = float(np.abs(p - g64).max())
            print("EPS handover q=%d mode %d: %d sequence left the scan, err %.3e" % (q, mode, n, err))
            assert n == 1 and err <= ec.TOL_GAMMA + (2.4e-7 * np.abs(ll64).max() if mode == engine.POST_LOG_NO_LL else 0)
            assert np.all(np.abs(ll - ll64) <= ec.tol_loglik(ll64))
        gamma = p if mode == engine.POST_PROB else engine.posterior(A, pi, E, eps=e)[0].cpu().numpy()[0]
        label, conf, _ = engine.posterior_decode(A, pi, E, eps=e)
        assert engine.exact_count(engine.OP_POSTERIOR, dims, tag=engine.DECODE_TAG) == 1
        assert np.array_equal(label.cpu().numpy()[0], gamma.argmax(-1).astype(np.uint8))
        assert np.array_equal(conf.cpu().numpy()[0], gamma.max(-1))
        with engine.option(engine.OPT_EXACT, engine.EXACT_OFF):
            off, _ = engine.posterior(A, pi, E, eps=e)
    err_off = float(np.abs(off.cpu().numpy()[0] - g64).max())
    print("EPS handover q=%d: unrouted err %.3e" % (q, err_off))
    assert err_off > 10 * ec.TOL_GAMMA


@pytest.mark.parametrize("spec", [s for s in ec.posterior_cases() if "thin" in s.models], ids=ec.spec_id)
def test_the_support_and_the_route_change_with_eps(spec):
    """The edge 0 -> D lies between 1e-16 and the case's eps: k_topo_check finds the model primitive at the default and
    routes it at the case's eps; both runs meet the oracle at their eps."""
    c = ec.build(spec)
    assert primitive(c["A"][0], ec.eps32(ec.CONTROL)) and not primitive(c["A"][0], ec.eps32(spec.eps))
    at_default, d0, g0, _ = route(spec, ec.CONTROL)
    at_eps, d1, g1, _ = route(spec, spec.eps)
    print("EPS route %s: %s %s at 1e-16, %s %s at its eps" % (ec.spec_id(spec), at_default, d0, at_eps, d1))
    assert at_eps == "model" and at_default != "model", (at_default, at_eps)
    r = ec.reference(spec)[0]
    assert np.abs(g1[0] - r["gamma"]).max() <= ec.TOL_GAMMA
    assert np.abs(g0[0] - r["control"]["gamma"]).max() <= ec.TOL_GAMMA


@pytest.mark.parametrize("spec", ec.refusal_cases(), ids=ec.spec_id)
def test_eps_below_the_domain_is_refused_by_every_entry_point(spec):
    """eps = 1e-20 and 1e-30 lie below HMM_EPS_MIN: HMM_ERR_BAD_ARGUMENT (-6) from every entry point of the sweep, and
    the same call is served at HMM_EPS_MIN itself."""
    c, e = ec.build(spec), ec.eps32(spec.eps)
    assert e < ec.EPS_MIN
    A, pi, E = dev(c["A"]), dev(c["pi"]), dev(c["E"])
    G = torch.ones_like(E)
    calls = [lambda eps: engine.posterior(A, pi, E, eps=eps), lambda eps: engine.forward(A, pi, E, eps=eps),
             lambda eps: engine.forward(A, pi, E, want_log_alpha=False, eps=eps),
             lambda eps: engine.backward(A, E, eps=eps), lambda eps: engine.posterior_decode(A, pi, E, eps=eps),
             lambda eps: engine.posterior_grad(A, pi, E, G, eps=eps)]
    if spec.L >= 641:                                        # (a shape the per-chunk plan of either width accepts)
        calls.append(lambda eps: engine.posterior_grad_scan(A, pi, E, G, eps=eps))
    for n, call in enumerate(calls):
        with pytest.raises(engine.EngineError, match=r"code -6"):
            call(e)
        with pytest.raises(engine.EngineError, match=r"code -6"):
            call(0.0)
        call(ec.EPS_MIN * 1.0001)                            # (the fp32 value just above the bound)
    torch.cuda.synchronize()
    # ... and at the lower bound every output of the sweep is held to the oracle
    lo = ec.eps32(ec.EPS_MIN * 1.0001)
    at = spec._replace(eps=ec.EPS_MIN)
    r = ec.oracle64(c["A"][0], c["pi"][0], c["E"][0], lo)
    tol_ll = ec.tol_loglik(r["ll"])
    ok = []
    with options(spec):
        for mode, name in zip(MODES, ("prob", "log", "log+ll")):
            out, ll = engine.posterior(A, pi, E, mode=mode, eps=lo)
            got, ll = out.cpu().numpy()[0], ll.cpu().numpy()[0]
            tol = ec.TOL_GAMMA
            if mode == engine.POST_LOG_NO_LL:
                got, tol = got - ll[:, None, None], tol + 2.4e-7 * np.abs(r["ll"]).max()
            p = got if mode == engine.POST_PROB else np.exp(got)
            ok.append(report("m=0", at, "gamma/" + name, float(np.abs(p - r["gamma"]).max()), tol))
            ok.append(report("m=0", at, "loglik/" + name, float((np.abs(ll - r["ll"]) / tol_ll).max()), 1.0))
        gamma = engine.posterior(A, pi, E, eps=lo)[0].cpu().numpy()
        la, ll_f = engine.forward(A, pi, E, eps=lo)
        _, ll_l = engine.forward(A, pi, E, want_log_alpha=False, eps=lo)
        lb = engine.backward(A, E, eps=lo)
        label, conf, ll_d = engine.posterior_decode(A, pi, E, eps=lo)
        for name, ll in (("forward", ll_f), ("loglik-only", ll_l), ("decode", ll_d)):
            ok.append(report("m=0", at, "loglik/" + name, float((np.abs(ll.cpu().numpy()[0] - r["ll"]) / tol_ll).max()), 1.0))
        assert_log_close_in_probability_space(la.cpu().numpy()[0], r["la"], (ec.spec_id(at), "log alpha"))
        assert_log_close_in_probability_space(lb.cpu().numpy()[0], r["lb"], (ec.spec_id(at), "log beta"))
        assert np.array_equal(label.cpu().numpy(), gamma.argmax(-1).astype(np.uint8))
        assert np.array_equal(conf.cpu().numpy(), gamma.max(-1))
        Gn = np.random.default_rng(spec.q).standard_normal(c["E"].shape).astype(np.float32)
        entries = [("posterior_grad/chunk", engine.posterior_grad, 1), ("posterior_grad/whole", engine.posterior_grad, 0)]
        if spec.L >= 641 and spec.q > 16:
            entries.append(("posterior_grad_scan", engine.posterior_grad_scan, 1))
        for log in (False, True):
            want = pm.oracle(c["A"][0], c["pi"][0], c["E"][0], Gn[0], log, eps=lo)
            for name, fn, pgchunk in entries:
                with engine.option(engine.OPT_PGCHUNK, pgchunk):
                    got = [t.cpu().numpy()[0] for t in fn(A, pi, E, dev(Gn), mode=engine.POST_LOG if log else engine.POST_PROB,
                                                          eps=lo)]
                present = c["A"][0] > 0                      # (absent edges per chunk: tests/postgrad_small_cases.py)
                got[0] = np.where(present, got[0], want[0]) if pgchunk else got[0]
                err = pm.errors(got, want, c["A"][0])[0]["tensor"]
                ok.append(report("m=0", at, "%s/%s tensor norm" % (name, "log" if log else "prob"), err, pm.TENSOR_REL))
                assert np.all(got[2][c["E"][0] <= np.float32(lo)] == 0.0)
    assert all(ok), ec.spec_id(at)


@pytest.mark.parametrize("spec", ec.decode_cases(), ids=ec.spec_id)
def test_decode_with_a_class_map(spec):
    """Against fp64 class sums of the oracle's gamma at the case's eps under the rule of
    tests/test_posterior_decode_gpu.py: |conf - conf64| <= n_max 2e-5, labels equal where the oracle's margin exceeds
    twice that (at least 99 % of the positions: tests/test_eps_sweep_cpu.py)."""
    c, ref, e = ec.build(spec), ec.reference(spec), ec.eps32(spec.eps)
    table, C, n_max = ec.class_map(spec)
    with options(spec):
        label, conf, ll = engine.posterior_decode(dev(c["A"]), dev(c["pi"]), dev(c["E"]), state_class=table,
                                                  num_classes=C, eps=e)
    label, conf, ll = label.cpu().numpy(), conf.cpu().numpy(), ll.cpu().numpy()
    for m, r in enumerate(ref):
        want, conf64, margin = dref.decode(r["gamma"], table, C)
        sure = margin > ec.decode_margin_rule(n_max)
        ok = report("m=%d" % m, spec, "conf", float(np.abs(conf[m] - conf64).max()), n_max * ec.TOL_GAMMA)
        print("EPS m=%d %s labels: %.4f of the positions compared" % (m, ec.spec_id(spec), sure.mean()))
        assert ok and sure.mean() >= 0.99
        assert np.array_equal(label[m][sure], want[sure]), (ec.spec_id(spec), m)
        assert np.all(np.abs(ll[m] - r["ll"]) <= ec.tol_loglik(r["ll"])), (ec.spec_id(spec), m)


@pytest.mark.parametrize("g", ec.grad_cases(), ids=ec.gspec_id)
def test_posterior_grad_at_the_callers_eps(g):
    """hmm_posterior_grad per chunk (HMM_OPT_PGCHUNK 1) and by the whole-sequence sweeps (0), hmm_posterior_grad_scan;
    dE is exactly 0 wherever E <= float32(eps)."""
    spec, e = g.spec, ec.eps32(g.spec.eps)
    c, G, ref = ec.build(spec), ec.grad_input(g), ec.grad_reference(g)
    args = (dev(c["A"]), dev(c["pi"]), dev(c["E"]), dev(G))
    mode = engine.POST_LOG if g.log else engine.POST_PROB
    dims = c["E"].shape
    with options(spec), engine.option(engine.OPT_PGCHUNK, 1 if g.route != "whole" else 0):
        if g.route == "scan":
            got = engine.posterior_grad_scan(*args, mode=mode, eps=e)
            serial = engine.posterior_grad_scan_serial_count(dims)
        else:
            got = engine.posterior_grad(*args, mode=mode, eps=e)
            serial = engine.posterior_grad_serial_count(dims)
    print("EPS serial %s: %d of %d sequences by the whole-sequence sweeps" % (ec.gspec_id(g), serial, dims[0] * dims[1]))
    if g.route == "whole":
        assert serial == dims[0] * dims[1]
    got = [t.cpu().numpy() for t in got]
    failed = []
    for m, r in enumerate(ref):
        mine = [x[m] for x in got]
        assert all(np.isfinite(x).all() for x in mine), (ec.gspec_id(g), m)
        if g.route == "whole":
            err, _ = pm.errors(mine, r["want"], c["A"][m])
        else:                    # per chunk: absent edges of dA to ABSENT_REL (tests/postgrad_small_cases.py)
            err, _ = ps.errors(mine, r["want"], c["A"][m], per_chunk=serial < dims[0] * dims[1])
            lim_absent = ps.ABSENT_REL if serial < dims[0] * dims[1] else pm.TENSOR_REL
            print("EPS m=%d %s dA/absent err %.3e limit %.3e" % (m, ec.gspec_id(g), err["dA/absent"], lim_absent))
            if not err.pop("dA/absent") <= lim_absent:
                failed.append((m, "dA/absent"))
        for norm, lim in r["limit"].items():
            print("EPS m=%d %s %s err %.3e limit %.3e e32 %.3e (%.3f)" % (m, ec.gspec_id(g), norm, err[norm], lim,
                                                                          r["e32"][norm], err[norm] / lim))
            if not err[norm] <= lim:
                failed.append((m, norm, err[norm], lim))
        clamped = c["E"][m] <= np.float32(e)
        assert clamped.any() == (spec.emis != "plain") and np.all(mine[2][clamped] == 0.0), (ec.gspec_id(g), m)
        if spec.emis == "edge":                              # the strict comparison: E == eps is clamped, its upper
            above = c["E"][m] == np.nextafter(np.float32(e), np.float32(1))     # neighbour is not
            assert (c["E"][m] == np.float32(e)).any() and above.any()
            assert np.array_equal(mine[2][above] != 0.0, r["want"][2][above] != 0.0), (ec.gspec_id(g), m)
    assert not failed, (ec.gspec_id(g), failed)


def test_layer_with_a_cell_epsilon():
    """cell.epsilon = 1e-6 on the 15-state gene layer: state_posterior_log_probs and the log-likelihood against the
    fp64 oracle at that eps on the layer's own A, pi, E."""
    from hmm_layer_amd import MsaHMMLayer as layer_module
    from oracle import textbook
    from test_layer_gpu import gene_setup
    b, L = 3, 300
    cell, x, _, _, _ = gene_setup(b, L, seed=5)
    cell.epsilon = 1e-6
    layer = layer_module.MsaHmmLayer(cell, use_prior=False)
    layer.build(x.shape)
    with torch.no_grad():
        A, pi, E = (t.cpu().numpy() for t in layer_module._engine_inputs(x, cell, None, False))
        logp = layer.state_posterior_log_probs(x).cpu().numpy()
        _, ll = layer.state_posterior_probs(x)
    e = ec.eps32(1e-6)
    g64, ll64 = textbook.posterior(A[0], pi[0], E[0], eps=e)
    moved = float(np.abs(g64 - textbook.posterior(A[0], pi[0], E[0])[0]).max())
    err = float(np.abs(np.exp(logp[0]) - g64).max())
    print("EPS layer: gamma err %.3e (limit 2e-5; the oracle moves by %.3e from eps = 1e-16)" % (err, moved))
    assert moved >= ec.DISCRIMINATING * ec.TOL_GAMMA
    assert err <= ec.TOL_GAMMA
    assert np.all(np.abs(ll.cpu().numpy()[0] - ll64) <= ec.tol_loglik(ll64))
