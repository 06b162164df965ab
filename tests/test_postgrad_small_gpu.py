"""hmm_posterior_grad for 1..16 states against the fp64 oracle: the whole-sequence sweeps (csrc/hmm_postgrad.inc,
k_pg_fb<16> / k_pg_adj<16>, k_pg_merge, k_pg_grad_sum, k_pg_sum_rows) and the per-chunk path that is the shipped
default there (csrc/hmm_postgrad_chunked.inc: k_pc_values, k_pc_src, k_pc_scan, k_pc_final, k_pc_fold /
k_pc_fold_seq).  Needs an MI355X.

Inputs, norms, limits and routing predictions: tests/postgrad_small_cases.py (the four norms of the 17..64-state
sweep; q = 1 under an absolute bound).  tests/test_postgrad_small_cpu.py shows from the oracle alone that the inputs
can carry this and that the table covers the edges it is for.  Every case runs under HMM_OPT_PGCHUNK = 0; every case
of two chunks or more under the shipped HMM_OPT_PGCHUNK = 1, with the serial count held against the prediction and the
sequences predicted "whole" bit-identical to the PGCHUNK = 0 run; the cases without a mixture clamp also under
HMM_OPT_PGCHUNK = 2 (per chunk for every sequence, no certificate; two and three chunks included).  dA entries of
absent edges: tensor norm in whole-sequence runs, 2e-2 of the oracle's largest dA entry where a model was served per
chunk (the exception include/hmm_engine.h states).  Each comparison prints its figures (pytest -s) before it asserts.

Worst error / limit measured on an MI355X over all cases of this file, per path and norm, with the largest e32 of the
norm (whole = served by the whole-sequence sweeps, chunk = models of which the per-chunk path served a sequence):
    whole  tensor     0.026  (7.7e-6 of 3e-4,    dense+triu-q5-b129-L64-plain-dense-prob-T16);    e32 <= 7.1e-6
    whole  dE/col     0.110  (6.4e-5 of 5.78e-4, gene+shipped-q15-b3-L203-plain-dense-prob-T16);  e32 <= 1.44e-4 (that case)
    whole  dE/seq     0.083  (2.50e-5 of 3e-4,   dense+triu-q5-b129-L64-plain-dense-prob-T16);    e32 <= 2.5e-5
    whole  dA/row     0.65   (1.95e-4 of 3e-4,   gene-q15-b2-L49-plain-dense-prob-T16);           e32 <= 1.8e-4 (gene+shipped, log)
    chunk  tensor     0.006  (1.8e-6 of 3e-4,    dense+sparse-q5-b2-L17-holes-dense-log)
    chunk  dE/col     0.069  (2.07e-5 of 3e-4,   gene-q15-b2-L80-plain-label-log-T16)
    chunk  dE/seq     0.012  (3.6e-6 of 3e-4,    gene-q15-b2-L80-plain-dense-prob-T16)
    chunk  dA/row     0.53   (1.59e-4 of 3e-4,   gene-q15-b3-L203-stretch-label-log-T16)
    chunk  dA/absent  1.3e-6 of the oracle's largest dA entry against the 2e-2 allowed (gene-q15-b2-L79-plain-dense-prob-T16)
The absent-edge entries of the per-chunk path are below 3e-4 everywhere in this sweep, by two orders: the 2e-2 exception
is not used by anything here (its stated cause, emissions of 1e-10 on the probable path across many chunks, is the
"rare" cases', which stay at 4e-7).  The serial count met the prediction exactly in every case (no case with an "open"
sequence under the shipped routing); the stretch sequence is the one redone whole in both modes.
q = 1: the engine returns exact zeros (before this sweep the sweeps left 1.08e-6 in dA against the bound of 1e-6).
"""
import functools

import numpy as np
import pytest
import torch

from hmm_layer_amd import engine

import postgrad_small_cases as pc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WORST = {}                                                   # (path, norm) -> (err / limit, err, limit, case)


def dev(x):
    return torch.as_tensor(np.array(x, dtype=np.float32, order="C"), device=DEV)    # (a copy: the cases are read-only)


def run(c, log, how, T=0, fn=engine.posterior_grad, count=engine.posterior_grad_serial_count):
    """-> (numpy dA, dpi, dE, sequences served by the whole-sequence sweeps) under HMM_OPT_PGCHUNK = how, chunk T."""
    with engine.option(engine.OPT_CHUNK, T), engine.option(engine.OPT_PGCHUNK, how):
        out = fn(dev(c["A"]), dev(c["pi"]), dev(c["E"]), dev(c["G"]), mode=engine.POST_LOG if log else engine.POST_PROB)
        n = count(c["E"].shape)
    return [t.cpu().numpy() for t in out], n


@functools.lru_cache(maxsize=8)
def whole(spec):
    """The case under HMM_OPT_PGCHUNK = 0 (every sequence by the whole-sequence sweeps)."""
    got, n = run(pc.build(spec), spec.log, 0, spec.T)
    assert n == len(spec.models) * spec.b
    return got


def check(spec, got, how, chunked_models=()):
    """`got` against the oracle under the four norms; chunked_models: the models the per-chunk path served."""
    c, ref, sid = pc.build(spec), pc.reference(spec), pc.spec_id(spec)
    failed = []
    for m, r in enumerate(ref):
        mine = [x[m] for x in got]
        assert all(np.isfinite(x).all() for x in mine), (sid, m)
        assert np.all(mine[2][c["E"][m] <= pc.EPS] == 0.0), (sid, m)                  # clamped emissions: exactly 0
        if spec.q == 1:                                      # the oracle's gradient is identically zero
            for name, x, lim in zip(("dA", "dpi", "dE"), mine, r["absolute"]):
                print("PGSMALL %s how=%d m=%d %s max|got| %.3e limit %.3e" % (sid, how, m, name, np.abs(x).max(), lim))
                if not np.abs(x).max() <= lim:
                    failed.append((m, name, float(np.abs(x).max()), lim))
            continue
        per_chunk = m in chunked_models
        err, _ = pc.errors(mine, r["want"], c["A"][m], per_chunk, pc.floor_columns(spec.models[m], c["A"][m]))
        lim = dict(pc.limits(r), **{"dA/absent": pc.ABSENT_REL if per_chunk else pc.TENSOR_REL})
        for norm in ("tensor",) + r["norms"] + ("dA/absent",):
            print("PGSMALL %s how=%d m=%d %s err %.3e limit %.3e e32 %.3e" % (sid, how, m, norm, err[norm], lim[norm],
                                                                              r["e32"].get(norm, 0.0)))
            key = ("chunk" if per_chunk else "whole", norm)
            if err[norm] / lim[norm] > WORST.get(key, (-1.0,))[0]:
                WORST[key] = (err[norm] / lim[norm], err[norm], lim[norm], sid)
            if not err[norm] <= lim[norm] and not (norm == "dA/absent" and not per_chunk):   # (whole: under "tensor")
                failed.append((m, norm, err[norm], lim[norm]))
    assert not failed, (sid, how, failed)


def served_per_chunk(spec, how, n):
    """The models of which the per-chunk path served a sequence in a run that left n to the whole-sequence sweeps."""
    if how == 0 or n == len(spec.models) * spec.b:
        return ()
    return tuple(m for m, r in enumerate(pc.routing(spec)) if r["primitive"])


@pytest.fixture(scope="module", autouse=True)
def record():
    yield
    for (path, norm), (ratio, err, lim, sid) in sorted(WORST.items()):
        print("PGSMALL-WORST %-5s %-9s %.3f (%.3e of %.3e, %s)" % (path, norm, ratio, err, lim, sid))


ALL = pc.all_specs()
CHUNKED = [s for s in ALL if pc.chunks(s) >= 2]


@pytest.mark.parametrize("spec", ALL, ids=pc.spec_id)
def test_whole_sequence_sweeps(spec):
    """Every case under HMM_OPT_PGCHUNK = 0."""
    got = whole(spec)
    check(spec, got, 0)
    if spec.L == 1:
        assert np.all(got[0] == 0.0)
    if spec.models[0] in ("fclamp", "fclamp2"):
        fclamp_edge(spec, got)


def fclamp_edge(spec, got):
    """The present edge 0 -> D into the clamped state (1e-20, or 1.25 eps) keeps what the backward recursion sends it."""
    D, rA = spec.q - 1, pc.reference(spec)[0]["want"][0]
    assert 0 < pc.build(spec)["A"][0, 0, D] < 2 * pc.EPS and rA[0, D] != 0.0
    print("PGSMALL %s edge 0->D got %.6e want %.6e" % (pc.spec_id(spec), got[0][0, 0, D], rA[0, D]))
    assert abs(got[0][0, 0, D] - rA[0, D]) <= 3e-4 * np.abs(rA).max()


@pytest.mark.parametrize("spec", CHUNKED, ids=pc.spec_id)
def test_shipped_routing(spec):
    """HMM_OPT_PGCHUNK = 1: the same norms whichever path served a sequence, the serial count inside what the fp64
    certificate and exposed-weight sums predict, and the sequences predicted "whole" bit-identical to PGCHUNK = 0."""
    c, n_all = pc.build(spec), len(spec.models) * spec.b
    got, n = run(c, spec.log, 1, spec.T)
    lo, hi = pc.serial_bounds(spec)
    print("PGSMALL %s how=1 whole-sequence %d of %d, predicted %d..%d" % (pc.spec_id(spec), n, n_all, lo, hi))
    check(spec, got, 1, served_per_chunk(spec, 1, n))
    assert lo <= n <= hi
    if spec.T and pc.chunks(spec) >= 2:                      # the forced chunk length is the one in force
        with engine.option(engine.OPT_CHUNK, spec.T), engine.option(engine.OPT_PGCHUNK, 2):
            assert engine.lib().hmm_posterior_grad_scan_chunk_len(*c["E"].shape) == spec.T == pc.chunk_len(spec)
    ser = whole(spec)
    for m, r in enumerate(pc.routing(spec)):
        for s, v in enumerate(r["verdict"]):
            if v == "whole" or not pc.shipped_per_chunk(spec):
                assert np.array_equal(got[2][m, s], ser[2][m, s]), (m, s)
    if spec.models[0] in ("fclamp", "fclamp2"):              # fclamp2 (PROB): through the per-chunk path
        fclamp_edge(spec, got)
        assert spec.models[0] == "fclamp" or spec.log or n == 0
    if spec.emis == "stretch":                               # its neighbours went per chunk
        assert n == 1 and not np.array_equal(got[2][0, 0], ser[2][0, 0])


@pytest.mark.parametrize("spec", [s for s in CHUNKED if pc.forced_per_chunk(s)], ids=pc.spec_id)
def test_every_sequence_per_chunk(spec):
    """HMM_OPT_PGCHUNK = 2 on the cases without a mixture clamp: no certificate, the arithmetic unaided."""
    got, n = run(pc.build(spec), spec.log, 2, spec.T)
    assert n == 0
    check(spec, got, 2, tuple(range(len(spec.models))))


@pytest.mark.parametrize("spec", pc.batch_sweep(), ids=pc.spec_id)
def test_each_sequence_alone(spec):
    """Whole-sequence sweeps: a sequence's dE is that of the sequence run alone, bit for bit."""
    c, got = pc.build(spec), whole(spec)
    for s in range(spec.b):
        alone, _ = run(dict(c, E=c["E"][:, s:s + 1], G=c["G"][:, s:s + 1]), spec.log, 0)
        assert np.array_equal(alone[2][:, 0], got[2][:, s]), s


@pytest.mark.parametrize("how", [0, 1])
def test_scan_entry_point_forwards(how):
    """hmm_posterior_grad_scan at q <= 16 is hmm_posterior_grad: the same bits and the same serial count."""
    spec = [s for s in pc.clamp_cases() if s.emis == "stretch" and not s.log][0]
    c = pc.build(spec)
    a, na = run(c, spec.log, how, spec.T)
    b, nb = run(c, spec.log, how, spec.T, engine.posterior_grad_scan, engine.posterior_grad_scan_serial_count)
    assert na == nb == (len(spec.models) * spec.b if how == 0 else 1)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
