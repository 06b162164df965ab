"""The sequence-sharded posterior (hmm_seqshard_reduce / hmm_seqshard_posterior, csrc/hmm_seqshard.inc) against its
fp64 restatement and the unsharded oracle, on one GPU: the R time slabs of a batch go through the engine's entry points
one after the other, as in tests/test_seqshard_gpu.py.  Needs an MI355X.

Inputs, norms and limits: tests/seqshard_cases.py; tests/test_seqshard_sweep_cpu.py shows from the reference alone that
they can carry the comparison.  Every comparison prints its figures (pytest -s) before it asserts.

  A  the slab operator alone against RefBackend.reduce, per column relative to the column's largest entry, limit
     max(4 e32, 1e-6); gene models with the compiled topology and with OPT_FORCE_DENSE = 1, which must differ in bits;
  B  benign inputs end to end over seven cut lists and three output modes: oracle <= 2e-5, unsharded engine <= 2e-6,
     every rank's log-likelihood accurate AND bit-identical to every other rank's, no flags;
  C  hard inputs: every sequence is flagged or accurate, the flags equal the reference's on the robust set, the sparse
     reduce's mark is reported by the slab that holds it, non-primitive models report phi = +inf on every rank;
  D  determinism, workspace reuse across shapes, no stale mark or psi, no mark read for a dense model.

Worst error / limit measured on an MI355X over all cases of this file:
    A  operator      0.57  (5.67e-7 of 1e-6,    d1-Ls100-start1-tiny-chunk0);  largest error 6.4e-6 of 1.31e-5
                           (g7-Ls1000-start0-tiny-chunk16, either reduce); e32 <= 4.0e-6
    B  oracle        0.53  (1.69e-4 of 3.18e-4, g7-L1513-cuts513 POST_LOG_NO_LL dense reduce); the other two modes 0.07
                           (1.46e-6 of 2e-5, g15+d15-L203 one rank POST_LOG)
    B  unsharded     0.81  (1.63e-6 of 2e-6,    g15+d15-L203-cuts1 POST_LOG)
    C  unflagged     0.48  (unsharded, 9.5e-7 of 2e-6, g15 POST_LOG dense reduce); oracle 0.38 (3.23e-5 of 8.48e-5, g7
                           POST_LOG_NO_LL dense reduce)
The deliberate edits of the kernels that this file was checked against (numbers only, on a scratch copy): reduce with
seq_start = 1 always 48 tests red, no entry prefix 29, the suffix of the next slab 29, the final compose without the
last chunk 49, phi without the reduce's mark 6, no copy of the global log-likelihood 28.
"""
import contextlib

import numpy as np
import pytest
import torch

from hmm_layer_amd import engine

import seqshard_cases as sc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODES = (engine.POST_PROB, engine.POST_LOG, engine.POST_LOG_NO_LL)


def dev(x, dtype=np.float32):
    return torch.as_tensor(np.array(x, dtype=dtype, order="C"), device=DEV)       # (a copy: the cases are read-only)


@contextlib.contextmanager
def options(chunk=0, force_dense=0):
    with engine.option(engine.OPT_CHUNK, chunk), engine.option(engine.OPT_FORCE_DENSE, force_dense):
        yield


def forces(name):
    return (0, 1) if sc.compiled(name) else (0,)


def bits(x):
    return np.ascontiguousarray(x).view(np.uint8)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


# ---- A: the slab operator -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sc.SWEEP_MODELS)
def test_slab_operator_against_the_restatement(name):
    A, _ = sc.model(name)
    q = A.shape[-1]
    Ad = dev(A)
    failed, worst, differ = [], (-1.0, ""), 0
    for spec in sc.a_cases((name,)):
        ref = sc.a_reference(spec)
        Ed = dev(sc.a_build(spec))
        got = {}
        for force in forces(name):
            with options(spec.chunk, force):
                op, ex = engine.seqshard_reduce(Ad, Ed, spec.seq_start, 2)
            op, ex = op.cpu().numpy(), ex.cpu().numpy()
            assert op.shape == ref["op"].shape and ex.shape == ref["ex"].shape
            assert np.isfinite(op).all(), (sc.a_id(spec), force)
            err = sc.op_error(op, ex, ref["op"], ref["ex"], q)
            print("SSWEEP-A %s dense=%d err %.3e limit %.3e e32 %.3e" % (sc.a_id(spec), force, err, ref["limit"], ref["e32"]))
            if not err <= ref["limit"]:
                failed.append((sc.a_id(spec), force, err, ref["limit"]))
            worst = max(worst, (err / ref["limit"], "%s dense=%d err %.3e" % (sc.a_id(spec), force, err)))
            if not ((op[..., q:, :] == 0).all() and (op[..., :, q:] == 0).all()):       # pad rows and columns: zero
                failed.append((sc.a_id(spec), force, "pad rows / columns of the operator are not zero"))
            got[force] = (op, ex)
        if len(got) == 2:
            differ += not (same_bits(got[0][0][..., :q, :q], got[1][0][..., :q, :q])
                           and same_bits(got[0][1][..., :q], got[1][1][..., :q]))
    print("SSWEEP-A %s worst err/limit %.3f (%s)" % ((name,) + worst))
    assert not failed, failed
    if sc.compiled(name):
        assert_compiled_topology_serves(name, differ)


SAME_BITS = ("g7",)


def assert_compiled_topology_serves(name, differ):
    """OPT_FORCE_DENSE really switches the reduce kernel of this model, so both were under test.  The dense reduce rounds
    differently somewhere in the operators of the 15-state model.  It does not for the 7-state one (measured: every
    operator of every case bit-identical; no state of that topology has more than three sources, and the MFMA adds its
    zeros exactly), so there the witness is the mark that the sparse reduce alone leaves on a chunk with two all-zero
    emission rows between two column sums."""
    assert differ > 0 or name in SAME_BITS, name
    A, pi = sc.model(name)
    E = np.array(sc.b_build(name, sc.B_L)[:, :, :64])
    E[:, :, 10:12] = 0.0
    phi = {}
    for force in (0, 1):
        with options(16, force):
            phi[force] = np.sum(sc.sharded_full(A, pi, E, [0, 64])["phis"], axis=0)
    gene = [m for m, n in enumerate(name.split("+")) if sc.compiled(n)]
    assert (phi[0][gene] >= 1).all() and (phi[1] <= sc.PHI_LIMIT).all(), (name, phi)


# ---- B: benign inputs end to end ------------------------------------------------------------------------------------
_unsharded = {}


def unsharded(name, kind, L, mode, force):
    """The unsharded engine call on a whole batch: computed once per (batch, mode, reduce), read-only."""
    key = (name, kind, L, mode, force)
    if key not in _unsharded:
        A, pi = sc.model(name)
        E = sc.b_build(name, L) if kind == "b" else sc.c_build(name)[0]
        with options(16, force):
            out, ll = engine.posterior(dev(A), dev(pi), dev(E), mode=mode)
        _unsharded[key] = sc._frozen(out.cpu().numpy(), ll.cpu().numpy())
    return _unsharded[key]


def as_gamma(out, ll, mode):
    """Posterior probabilities from an output of `mode` (ll: (k,b) log-likelihoods for POST_LOG_NO_LL)."""
    if mode == engine.POST_PROB:
        return out.astype(np.float64)
    if mode == engine.POST_LOG:
        return np.exp(out.astype(np.float64))
    return np.exp(out.astype(np.float64) - ll[..., None, None])


def accuracy(res, mode, g64, ll64, ref, llref, seqs=None):
    """-> list of (what, figure, limit) that a sharded result misses on the sequences `seqs` (k,b bool; default all)."""
    seqs = np.ones(ll64.shape, bool) if seqs is None else seqs
    extra = sc.NO_LL_REL * np.abs(ll64).max() if mode == engine.POST_LOG_NO_LL else 0.0
    got = as_gamma(res["out"], res["lls"][0], mode)
    checks = [("oracle", np.abs(got - g64).max((2, 3)), sc.GAMMA_TOL + extra),
              ("unsharded", np.abs(got - as_gamma(ref, llref, mode)).max((2, 3)), sc.UNSHARDED_TOL + extra)]
    for r, ll in enumerate(res["lls"]):
        checks.append(("loglik rank %d" % r, np.abs(ll - ll64) - sc.LL_REL * np.abs(ll64), sc.LL_ABS))
    missed = []
    for what, fig, lim in checks:
        fig = np.where(np.isnan(fig), np.inf, fig)
        if seqs.any() and not (fig[seqs] <= lim).all():
            missed.append((what, float(fig[seqs].max()), lim))
    return missed, {what: (float(fig[seqs].max()) if seqs.any() else 0.0, lim) for what, fig, lim in checks[:2]}


def ranks_agree(res):
    """Every rank's whole-sequence log-likelihood is bit-identical to rank 0's (per sequence: (k,b) bool)."""
    ok = np.ones(res["lls"][0].shape, bool)
    for ll in res["lls"][1:]:
        ok &= ll.view(np.int64) == res["lls"][0].view(np.int64)
    return ok


@pytest.mark.parametrize("name", sc.B_MODELS + tuple("%s@long" % m for m in sc.B_LONG_MODELS))
def test_benign_inputs_no_flags_and_accurate(name):
    long = name.endswith("@long")
    name = name[:-5] if long else name
    A, pi = sc.model(name)
    failed, worst = [], {}
    for spec in ([sc.B_LONG._replace(model=name)] if long else [s for s in sc.b_cases((name,)) if s.L == sc.B_L]):
        E = sc.b_build(name, spec.L)
        g64, ll64 = sc.oracle(name, "b", spec.L)
        for force in forces(name):
            for mode in MODES:
                ref, llref = unsharded(name, "b", spec.L, mode, force)
                with options(16, force):
                    res = sc.sharded_full(A, pi, E, list(spec.cuts), mode)
                tag = "%s mode=%d dense=%d" % (sc.b_id(spec), mode, force)
                assert len(res["lls"]) == len(spec.cuts) - 1 and res["out"].shape == E.shape
                missed, figs = accuracy(res, mode, g64, ll64, ref, llref)
                phi = np.sum(res["phis"], axis=0)
                print("SSWEEP-B %s oracle %.3e of %.3e unsharded %.3e of %.3e phi %.3e" % ((tag,) + figs["oracle"] + figs["unsharded"] + (phi.max(),)))
                for what, (v, lim) in figs.items():
                    worst[what] = max(worst.get(what, (-1.0, "")), (v / lim, "%s: %.3e of %.3e" % (tag, v, lim)))
                if missed:
                    failed.append((tag, missed))
                if not ranks_agree(res).all():
                    failed.append((tag, "log-likelihoods differ between ranks", [ll.tolist() for ll in res["lls"]]))
                if not (np.isfinite(phi).all() and (phi >= 0).all() and (phi <= sc.PHI_LIMIT).all()):
                    failed.append((tag, "flags", phi.tolist()))
    print("SSWEEP-B %s worst error / limit %s" % (name, worst))
    assert not failed, failed


# ---- C: hard inputs -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sc.C_MODELS)
def test_hard_inputs_are_flagged_or_accurate(name):
    A, pi = sc.model(name)
    E, lay = sc.c_build(name)
    g64, ll64 = sc.oracle(name, "c")
    failed = []
    for force in forces(name):
        for mode in MODES:
            ref, llref = unsharded(name, "c", sc.C_L, mode, force)
            with options(sc.C_CHUNK, force):
                res = sc.sharded_full(A, pi, E, list(sc.C_CUTS), mode)
            tag = "%s mode=%d dense=%d" % (name, mode, force)
            phi = np.sum(res["phis"], axis=0)
            assert not np.isnan(phi).any() and (np.asarray(res["phis"]) >= 0).all(), tag
            flagged = ~(phi <= sc.PHI_LIMIT)
            print("SSWEEP-C %s flagged %s" % (tag, np.flatnonzero(flagged[0]).tolist()))
            # the invariant: flagged, or as accurate as a benign input
            missed, figs = accuracy(res, mode, g64, ll64, ref, llref, ~flagged)
            print("SSWEEP-C %s unflagged: oracle %.3e of %.3e unsharded %.3e of %.3e" % ((tag,) + figs["oracle"] + figs["unsharded"]))
            if missed:
                bad = [i for i in np.flatnonzero(~flagged[0])
                       if accuracy(res, mode, g64, ll64, ref, llref, np.arange(len(lay))[None] == i)[0]]
                failed.append((tag, "unflagged and wrong", missed, [(i, lay[i], float(phi[0, i])) for i in bad]))
            if not ranks_agree(res).all():
                failed.append((tag, "log-likelihoods differ between ranks"))
            # what gather_flagged falls back to is right for the flagged ones
            got = as_gamma(ref, llref, mode)
            extra = sc.NO_LL_REL * np.abs(ll64).max() if mode == engine.POST_LOG_NO_LL else 0.0
            if flagged.any() and not np.abs(got - g64)[flagged].max() <= sc.GAMMA_TOL + extra:
                failed.append((tag, "unsharded call off the oracle on a flagged sequence"))
            # the flags are the reference's wherever its verdict is robust.  The sparse reduce's mark is not part of the
            # reference (it guards fp32's range, not the clamps): with the compiled topology it may flag a sequence
            # more, and then it shows as a whole 1 in phi and the dense reduce leaves the sequence unflagged
            rob = sc.ROBUST[name]
            wrong = [i for i in rob["flagged"] if not flagged[0, i]]
            more = [i for i in rob["unflagged"] if flagged[0, i]]
            if force == 0 and sc.compiled(name):
                wrong += [i for i in more if not phi[0, i] >= 1]
            else:
                wrong += more
            if wrong:
                failed.append((tag, "flags differ from the reference's", [(i, lay[i], float(phi[0, i])) for i in wrong]))
            # the sparse reduce's mark: reported by the slab that holds the two zero rows, by no other
            if force == 0 and sc.compiled(name):
                for i, h in enumerate(lay):
                    if h.kind == "mark":
                        per_slab = [float(p[0, i]) for p in res["phis"]]
                        print("SSWEEP-C %s mark in slab %d: phi per slab %s" % (tag, h.place, per_slab))
                        if not (per_slab[h.place] >= 1 and all(p <= sc.PHI_LIMIT for r, p in enumerate(per_slab) if r != h.place)):
                            failed.append((tag, "mark", h, per_slab))
    assert not failed, failed


@pytest.mark.parametrize("name", sc.C_NONPRIMITIVE)
def test_nonprimitive_models_are_flagged_on_every_rank(name):
    A, pi = sc.model(name)
    E, _ = sc.c_build(name)
    g64, _ = sc.oracle(name, "c")
    with options(sc.C_CHUNK, 0):
        res = sc.sharded_full(A, pi, E, list(sc.C_CUTS))
    for ph in res["phis"]:
        assert np.isposinf(ph).all(), (name, ph)
    ref, _ = unsharded(name, "c", sc.C_L, engine.POST_PROB, 0)
    assert np.abs(ref - g64).max() <= sc.GAMMA_TOL


# ---- D: hygiene -----------------------------------------------------------------------------------------------------
KEYS = ("out", "lls", "phis", "ops", "exs")


def same_result(a, b):
    """The entries of two sharded_full() results that differ in any bit."""
    def parts(res, key):
        return [res[key]] if key == "out" else res[key]
    return [key for key in KEYS if not all(same_bits(x, y) for x, y in zip(parts(a, key), parts(b, key)))]


def test_two_identical_runs_give_identical_bits():
    for name, E, cuts in (("g15", sc.b_build("g15", sc.B_L), sc.B_CUTS[5]), ("g15+d15", sc.b_build("g15+d15", sc.B_L), sc.B_CUTS[4]),
                          ("g7", sc.c_build("g7")[0], sc.C_CUTS)):
        A, pi = sc.model(name)
        with options(16, 0):
            first = sc.sharded_full(A, pi, E, list(cuts))
            second = sc.sharded_full(A, pi, E, list(cuts))
        assert same_result(first, second) == [], name


def test_workspace_reuse_across_shapes_on_one_stream():
    streams = [torch.cuda.Stream() for _ in range(5)]
    big, small = ("g15", sc.b_build("g15", sc.B_L), sc.B_CUTS[5]), ("d5", sc.b_build("d5", sc.B_L)[:, :2, :40], (0, 1, 40))
    runs = []
    with options(16, 0):
        for name, E, cuts in (big, small, big):
            A, pi = sc.model(name)
            runs.append(sc.sharded_full(A, pi, E, list(cuts), streams=streams[:len(cuts) - 1]))
    assert same_result(runs[0], runs[2]) == []
    # (the small call in between is right as well; a prefix of a sequence is a sequence of its own: against the engine)
    with options(16, 0):
        ref = engine.posterior(dev(sc.model("d5")[0]), dev(sc.model("d5")[1]), dev(small[1]))[0].cpu().numpy()
    assert runs[1]["out"].shape == (1, 2, 40, 5) and np.abs(runs[1]["out"] - ref).max() <= sc.UNSHARDED_TOL


def test_a_benign_call_after_a_marked_one_has_no_flags():
    """Same shape, same streams, hence the same workspaces: first the 15-state hard batch (clamp-decided sequences and
    the sparse reduce's marks), then uniform emissions; then a dense model of the same shape, for which the pad lane
    that carries the mark is an ordinary exponent that k_seqshard_phi must not read."""
    streams = [torch.cuda.Stream() for _ in range(3)]
    E, lay = sc.c_build("g15")
    benign = (np.random.default_rng(31).random(E.shape) * 0.9 + 0.05).astype(np.float32)
    with options(sc.C_CHUNK, 0):
        A, pi = sc.model("g15")
        hard = sc.sharded_full(A, pi, E, list(sc.C_CUTS), streams=streams)
        marks = [i for i, h in enumerate(lay) if h.kind == "mark"]
        assert (np.sum(hard["phis"], axis=0)[0, marks] >= 1).all()
        after = sc.sharded_full(A, pi, benign, list(sc.C_CUTS), streams=streams)
        phi = np.sum(after["phis"], axis=0)
        assert np.isfinite(phi).all() and (phi >= 0).all() and (phi <= sc.PHI_LIMIT).all(), phi
        A, pi = sc.model("d15")
        dense = sc.sharded_full(A, pi, benign, list(sc.C_CUTS), streams=streams)
        phi = np.sum(dense["phis"], axis=0)
        assert np.isfinite(phi).all() and (phi >= 0).all() and (phi <= sc.PHI_LIMIT).all(), phi
        # (the dense reduce does write that lane: the guard in k_seqshard_phi is what keeps it out of phi)
        ref = engine.posterior(dev(A), dev(pi), dev(benign))[0].cpu().numpy()
    assert np.abs(dense["out"] - ref).max() <= sc.UNSHARDED_TOL
