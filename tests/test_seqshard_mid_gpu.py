"""The sequence-sharded posterior for 17 to 64 states (hmm_seqshard_mid_reduce / hmm_seqshard_mid_posterior,
csrc/hmm_seqshard_mid.inc) against its fp64 restatement, the unsharded fp64 oracle and the unsharded engine, on one GPU:
the R time slabs of a batch go through the entry points one after the other, one stream (one workspace) per "rank", as
in tests/test_seqshard_sweep_gpu.py.  Needs an MI355X.

Inputs, norms and limits: tests/seqshard_mid_cases.py; tests/test_seqshard_mid_cpu.py shows from the restatement alone
that they can carry the comparison.  Every comparison prints its figures (pytest -s) before it asserts.

  A  the slab operator against RefBackend.reduce, per column relative to the column's largest entry after aligning the
     exponents, limit max(4 e32, 1e-6) with e32 the float32-numpy operator's error; exact-zero padding, all finite;
  B  benign batches end to end over five cut lists (and L = 1513 cut at 513) and three output modes: oracle gamma
     <= 2e-5 (POST_LOG_NO_LL + 2.4e-7 |ll|), log-likelihood 1e-6 |ll| + 2e-4 and bit-identical between the ranks, phi
     <= PHI_LIMIT; against the unsharded engine under HMM_EXACT_OFF at OPT_CHUNK 16: twice the spread of that engine
     over OPT_CHUNK 16 / 32 / 48 / 64 on the same batch, floor 2e-6 (POST_LOG_NO_LL + 2.4e-7 |ll|, as for 16 states; a
     cut is one more chunk boundary plus one compose rounding);
  C  hard inputs: flagged, or as accurate as a benign one; the flags are the restatement's; non-primitive models
     report phi = +inf on every rank with finite outputs; a reduce's mark is reported by the slab that holds it;
  D  R = 1 against engine.posterior bit for bit, repeated calls, workspace reuse, graph capture;
  E  MsaHMMLayer.state_posterior_log_probs_sharded on a 29-state cell, two slabs.

Worst error / limit measured on an MI355X over all cases of this file:
    A  operator   0.47  (2.53e-6 of 5.41e-6, g29-Ls513-start1-plain, the compiled reduce, two-level compose); the other
                        models 0.29 .. 0.38 (3.2e-7 .. 1.1e-6); e32 <= 3.9e-6
    B  oracle     0.40  (1.25e-4 of 3.12e-4, g29-L1513-cuts513 POST_LOG_NO_LL); POST_PROB / POST_LOG at most 0.07
                        (1.29e-6 of 2e-5, g43-L203 one rank POST_LOG)
    B  engine     0.84  (1.67e-6 of 2e-6, g43-L203 one rank POST_LOG: 203 positions of 43 states run engine.posterior
                        on the one-wave-per-sequence kernels, spread 0, the floor); where engine.posterior takes the
                        scan: 0.50 (1.58e-6 of 3.16e-6 = twice the spread, g29-L203-cuts50_120_202 POST_LOG dense
                        reduce), L = 1513: 0.41 (1.22e-4 of 2.94e-4, g29 POST_LOG_NO_LL; POST_PROB 2.98e-7 of 2e-6)
    C  unflagged  0.08  (oracle, 1.67e-6 of 2e-5, g43 state 10 POST_LOG); flagged sequences: phi 0.24 .. 0.83 as the
                        restatement's, + 1 per chunk the compiled reduce marked (g29: 2.83 = 0.83 + 2)
    D  R = 1      out bit-identical to engine.posterior (six models); log-likelihood within 1.2e-8 relative
    E  layer      1.17e-6 of 2e-6 (POST_LOG), 3.4e-4 with no_loglik (|ll| of 1.5e3 in fp32); the flagged sequence
                        bit-identical to the unsharded call after gather_flagged
"""
import contextlib

import numpy as np
import pytest
import torch

from hmm_layer_amd import engine, seqshard, seqshard_mid

import seqshard_mid_cases as mcs

pytestmark = pytest.mark.gpu
MODES = (engine.POST_PROB, engine.POST_LOG, engine.POST_LOG_NO_LL)
dev = mcs.dev


@contextlib.contextmanager
def options(chunk=16, force_dense=0, exact=None):
    with engine.option(engine.OPT_CHUNK, chunk), engine.option(engine.OPT_FORCE_DENSE, force_dense):
        if exact is None:
            yield
        else:
            with engine.option(engine.OPT_EXACT, exact):
                yield


def bits(x):
    return np.ascontiguousarray(x).view(np.uint8)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def as_gamma(out, ll, mode):
    if mode == engine.POST_PROB:
        return out.astype(np.float64)
    if mode == engine.POST_LOG:
        return np.exp(out.astype(np.float64))
    return np.exp(out.astype(np.float64) - ll[..., None, None])


def ranks_agree(res):
    return all(same_bits(ll, res["lls"][0]) for ll in res["lls"])


# ---- A: the slab operator -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", mcs.MODELS)
def test_a_slab_operator_against_the_restatement(name):
    A, _ = mcs.model(name)
    q, QT = A.shape[-1], mcs.tile(A.shape[-1])
    Ad = dev(A)
    failed, worst, differ = [], (-1.0, ""), 0
    got = {}
    for spec in [s for s in mcs.a_cases() if s.model == name]:
        ref = mcs.a_reference(spec)
        Ed = dev(mcs.a_build(spec))
        with options(spec.chunk, spec.dense):
            op, ex = seqshard_mid.reduce(Ad, Ed, spec.seq_start, 2)
        op, ex = op.cpu().numpy(), ex.cpu().numpy()
        assert op.shape == ref["op"].shape == A.shape[:1] + (mcs.B, QT, QT) and ex.shape == ref["ex"].shape
        assert np.isfinite(op).all(), mcs.a_id(spec)
        err = mcs.op_error(op, ex, ref["op"], ref["ex"], q)
        print("MID-A %s err %.3e limit %.3e e32 %.3e minexp %d" % (mcs.a_id(spec), err, ref["limit"], ref["e32"], ex.min()))
        if not err <= ref["limit"]:
            failed.append((mcs.a_id(spec), err, ref["limit"]))
        worst = max(worst, (err / ref["limit"], "%s err %.3e" % (mcs.a_id(spec), err)))
        if not ((op[..., q:, :] == 0).all() and (op[..., :, q:] == 0).all() and (ex[..., q:] == 0).all()):
            failed.append((mcs.a_id(spec), "the padding of the operator or of its exponents is not zero"))
        s = op[..., :q, :q].astype(np.float64).sum(-2)
        if not ((s > 0.4999) & (s < 1.0001)).all():
            failed.append((mcs.a_id(spec), "column sums outside [0.5, 1)", float(s.min()), float(s.max())))
        if spec.variant == "tiny" and spec.Ls == 1000 and not ex[..., :q].max() < -33000:
            failed.append((mcs.a_id(spec), "exponents", int(ex[..., :q].max())))
        key = spec._replace(dense=0)
        if key in got and spec.dense:
            differ += not same_bits(got[key], op)
        got[spec] = op
    print("MID-A %s worst err/limit %.3f (%s)" % ((name,) + worst))
    assert not failed, failed
    if name == "g29":
        assert differ > 0                                    # OPT_FORCE_DENSE switches the reduce kernel: both were run


# ---- B: benign batches end to end -----------------------------------------------------------------------------------
_cache = {}


def unsharded(name, L, mode, chunk, E=None, tag="b"):
    """engine.posterior on a whole batch under HMM_EXACT_OFF: once per (batch, mode, chunk), read-only."""
    key = (name, L, mode, chunk, tag)
    if key not in _cache:
        A, pi = mcs.model(name)
        E = mcs.b_build(name, L) if E is None else E
        with options(chunk, 0, engine.EXACT_OFF):
            out, ll = engine.posterior(dev(A), dev(pi), dev(E), mode=mode)
        _cache[key] = mcs._frozen(out.cpu().numpy(), ll.cpu().numpy())
    return _cache[key]


def engine_limit(name, L, mode, E=None, tag="b"):
    """-> (the unsharded engine's gamma at OPT_CHUNK 16, the limit against it: twice its spread over OPT_CHUNK 16, 32,
    48, 64; the floor is the 16-state family's limit as tests/test_seqshard_sweep_gpu.py has it, 2e-6, for POST_LOG_NO_LL
    plus fp32's resolution of values of the log-likelihood's size, 2.4e-7 |ll|.  Batches of 33..64 states shorter than
    256 positions run engine.posterior on the one-wave-per-sequence kernels, which have no chunks: spread 0, the floor)."""
    out16, ll16 = unsharded(name, L, mode, 16, E, tag)
    ref = as_gamma(out16, ll16, mode)
    spread = max(float(np.abs(as_gamma(*unsharded(name, L, mode, c, E, tag), mode) - ref).max()) for c in (32, 48, 64))
    floor = 2e-6 + (mcs.NO_LL_REL * float(np.abs(ll16).max()) if mode == engine.POST_LOG_NO_LL else 0.0)
    return ref, max(2 * spread, floor), spread


def benign_checks(name, E, cuts, mode, force, g64, ll64, L, tag="b"):
    A, pi = mcs.model(name)
    with options(16, force):
        res = mcs.sharded_full(A, pi, E, list(cuts), mode)
    what = "%s L%d cuts %s mode=%d dense=%d" % (name, L, "_".join(map(str, cuts[1:-1])) or "none", mode, force)
    assert len(res["lls"]) == len(cuts) - 1 and res["out"].shape == E.shape
    extra = mcs.NO_LL_REL * np.abs(ll64).max() if mode == engine.POST_LOG_NO_LL else 0.0
    got = as_gamma(res["out"], res["lls"][0], mode)
    e_or = float(np.abs(got - g64).max())
    ref, lim, spread = engine_limit(name, L, mode, E if tag != "b" else None, tag)
    e_un = float(np.abs(got - ref).max())
    e_ll = max(float((np.abs(ll - ll64) - mcs.LL_REL * np.abs(ll64)).max()) for ll in res["lls"])
    phi = np.sum(res["phis"], axis=0)
    print("MID-B %s oracle %.3e of %.3e engine %.3e of %.3e (spread %.3e) loglik %.3e of %.3e phi %.3e"
          % (what, e_or, mcs.GAMMA_TOL + extra, e_un, lim, spread, e_ll, mcs.LL_ABS, phi.max()))
    missed = []
    if not e_or <= mcs.GAMMA_TOL + extra:
        missed.append(("oracle", e_or))
    if not e_un <= lim:
        missed.append(("engine", e_un, lim))
    if not e_ll <= mcs.LL_ABS:
        missed.append(("loglik", e_ll))
    if not ranks_agree(res):
        missed.append("log-likelihoods differ between ranks")
    if not (np.isfinite(phi).all() and (phi >= 0).all() and (phi <= mcs.PHI_LIMIT).all()):
        missed.append(("flags", phi.tolist()))
    figs = dict(oracle=e_or / (mcs.GAMMA_TOL + extra), engine=e_un / lim)
    return ([(what, missed)] if missed else []), figs, what


@pytest.mark.parametrize("name", mcs.MODELS + tuple("%s@long" % m for m in mcs.B_LONG_MODELS))
def test_b_benign_batches_end_to_end(name):
    long = name.endswith("@long")
    name = name[:-5] if long else name
    L = mcs.B_LONG_L if long else mcs.B_L
    E = mcs.b_build(name, L)
    g64, ll64 = mcs.oracle(name, L)
    failed, worst = [], {}
    for cuts in ((mcs.B_LONG_CUTS,) if long else mcs.B_CUTS):
        for force in ((0, 1) if name == "g29" else (0,)):
            for mode in MODES:
                bad, figs, what = benign_checks(name, E, cuts, mode, force, g64, ll64, L)
                failed += bad
                for k, v in figs.items():
                    worst[k] = max(worst.get(k, (-1.0, "")), (v, what))
    print("MID-B %s worst error / limit %s" % (name, worst))
    assert not failed, failed


# ---- C: hard inputs -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,state,cuts", mcs.C_CASES, ids=mcs.c_id)
def test_c_hard_inputs_are_flagged_or_accurate(name, state, cuts):
    A, pi = mcs.model(name)
    E = mcs.c_build(name, state)
    g64, ll64 = mcs.c_oracle(name, state)
    _, ref_phi, ref_flags = mcs.c_reference(name, state, cuts)
    failed = []
    for force in ((0, 1) if name == "g29" else (0,)):
        for mode in MODES:
            with options(16, force):
                res = mcs.sharded_full(A, pi, E, list(cuts), mode)
            tag = "%s state %d cuts %s mode=%d dense=%d" % (name, state, cuts, mode, force)
            phi = np.sum(res["phis"], axis=0)[0]
            assert not np.isnan(phi).any() and (np.asarray(res["phis"]) >= 0).all(), tag
            flagged = ~(phi <= mcs.PHI_LIMIT)
            extra = mcs.NO_LL_REL * np.abs(ll64).max() if mode == engine.POST_LOG_NO_LL else 0.0
            got = as_gamma(res["out"], res["lls"][0], mode)
            err = np.abs(got - g64).max((0, 2, 3))
            ell = np.max([np.abs(ll - ll64)[0] - mcs.LL_REL * np.abs(ll64)[0] for ll in res["lls"]], axis=0)
            print("MID-C %s phi %s (restatement %s) oracle %s of %.3e loglik %s" % (tag, phi, ref_phi, err, mcs.GAMMA_TOL + extra, ell))
            # (no NaN; a log posterior may be -inf where the probability is below fp32's range, as in hmm_posterior)
            if np.isnan(res["out"]).any() or (mode == engine.POST_PROB and not np.isfinite(res["out"]).all()):
                failed.append((tag, "not finite"))
            ok = flagged | ((err <= mcs.GAMMA_TOL + extra) & (ell <= mcs.LL_ABS))
            if not ok.all():
                failed.append((tag, "unflagged and wrong", phi.tolist(), err.tolist()))
            # the flags are the restatement's.  A reduce's mark is not part of the restatement (it guards fp32's range,
            # not the clamps): it may flag a sequence more, and then it shows as a whole 1 in phi
            if (ref_flags & ~flagged).any() or (flagged & ~ref_flags & ~(phi >= 1)).any():
                failed.append((tag, "flags differ from the restatement's", phi.tolist(), ref_phi.tolist()))
            if not ranks_agree(res):
                failed.append((tag, "log-likelihoods differ between ranks"))
    assert not failed, failed


@pytest.mark.parametrize("name", mcs.NONPRIMITIVE)
def test_c_non_primitive_models_report_inf_on_every_rank(name):
    A, pi = mcs.model(name)
    E = mcs.b_build(name, 100)
    for mode in MODES:
        with options(16):
            res = mcs.sharded_full(A, pi, E, [0, 33, 50, 100], mode)
        print("MID-C %s mode=%d phi %s" % (name, mode, [p.tolist() for p in res["phis"]]))
        for p in res["phis"]:
            assert np.isposinf(p).all()
        assert np.isfinite(res["out"]).all() and np.isfinite(np.asarray(res["lls"])).all()
        for op in res["ops"]:
            assert np.isfinite(op).all()


@pytest.mark.parametrize("name,force", [("g29", 0), ("g29", 1), ("d33", 0)])
def test_c_zero_rows_inside_a_chunk_are_marked_by_their_slab(name, force):
    """Two all-zero emission rows at chunk positions (10, 11) of the middle slab: between two column sums of the sparse
    reduce the columns lose 2^-106 and the chunk is marked; the dense reduces mark an observation that every column
    survives at the floor only.  Either way the slab that holds the rows reports a whole 1 or more, the others stay
    below the limit, and everything is finite."""
    A, pi = mcs.model(name)
    E = np.array(mcs.b_build(name, mcs.B_L)[:, :, :96])
    E[:, 1, 42:44] = 0.0
    for mode in MODES:
        with options(16, force):
            res = mcs.sharded_full(A, pi, E, [0, 32, 64, 96], mode)
        per_slab = [p[0].tolist() for p in res["phis"]]
        print("MID-C %s dense=%d mode=%d zero rows: phi per slab %s" % (name, force, mode, per_slab))
        assert not np.isnan(res["out"]).any() and np.isfinite(np.asarray(res["lls"])).all()
        assert np.isfinite(res["out"][:, [0, 2]]).all()
        for r, p in enumerate(res["phis"]):
            assert (p[0, [0, 2]] <= mcs.PHI_LIMIT).all()
            assert (p[0, 1] >= 1) if r == 1 else (p[0, 1] < 1)
        for op in res["ops"]:
            assert np.isfinite(op).all()


# ---- D: regressions and contract ------------------------------------------------------------------------------------
D_L = 272                                                    # 17 chunks of 16; 33..64 states take engine.posterior's scan


@pytest.mark.parametrize("name,force", [("g29", 0), ("g29", 1), ("d32", 0), ("d33", 0), ("g43", 0), ("d64", 0)])
def test_d_single_rank_equals_the_unsharded_call(name, force):
    """R = 1, POST_PROB: out is engine.posterior's under HMM_EXACT_OFF and the same chunk, bit for bit — the same chunk
    operators, the same hops from pi and from ones, the same apply kernels.  (The log-likelihood is the hop's over the
    composed slab operator: one compose rounding away.)  Three runs: bit-identical to each other."""
    A, pi = mcs.model(name)
    E = mcs.b_build(name, D_L)
    with options(16, force, engine.EXACT_OFF):
        want, ll = engine.posterior(dev(A), dev(pi), dev(E), mode=engine.POST_PROB)
    want, ll = want.cpu().numpy(), ll.cpu().numpy()
    with options(16, force):
        runs = [mcs.sharded_full(A, pi, E, [0, D_L], engine.POST_PROB) for _ in range(3)]
    d = float(np.abs(runs[0]["out"] - want).max())
    dl = float((np.abs(runs[0]["lls"][0] - ll) / np.abs(ll)).max())
    print("MID-D %s dense=%d R=1: max |out - engine.posterior| %.3e, loglik rel %.3e" % (name, force, d, dl))
    assert same_bits(runs[0]["out"], want)
    assert dl <= 1e-6
    for run in runs[1:]:
        for key in ("out",):
            assert same_bits(run[key], runs[0][key])
        for key in ("lls", "phis", "ops", "exs"):
            assert same_bits(run[key][0], runs[0][key][0]), key


def test_d_workspace_reuse_across_shapes_and_widths():
    """One set of streams (hence workspaces) for everything: a marked batch, then other shapes and the other width,
    then a benign batch of the first shape — no stale phi, no stale mark."""
    streams = [torch.cuda.Stream() for _ in range(3)]
    A, pi = mcs.model("g29")
    E = np.array(mcs.b_build("g29", mcs.B_L)[:, :, :96])
    hard = E.copy()
    hard[:, :, 42:44] = 0.0
    with options(16):
        first = mcs.sharded_full(A, pi, E, [0, 32, 64, 96], 0, streams)
        marked = mcs.sharded_full(A, pi, hard, [0, 32, 64, 96], 0, streams)
        assert (np.sum(marked["phis"], axis=0) >= 1).all()
        for other, L in (("d64", 100), ("d17", 40), ("g29+d29", 203)):
            Ao, pio = mcs.model(other)
            mcs.sharded_full(Ao, pio, mcs.b_build(other, mcs.B_L)[:, :, :L], [0, L // 3, L // 2, L], 1, streams)
        again = mcs.sharded_full(A, pi, E, [0, 32, 64, 96], 0, streams)
    assert (np.sum(again["phis"], axis=0) <= mcs.PHI_LIMIT).all()
    for key in ("out",):
        assert same_bits(again[key], first[key])
    for key in ("lls", "phis", "ops", "exs"):
        for r in range(3):
            assert same_bits(again[key][r], first[key][r]), (key, r)


@pytest.mark.parametrize("name", ["g29", "d33"])
def test_d_two_calls_captured_into_one_graph(name):
    """reduce -> posterior of one rank (R = 1) on one stream, captured once and replayed: no host synchronisation, no
    helper stream; bit-identical to the eager calls."""
    A, pi = (dev(x) for x in mcs.model(name))
    E = dev(mcs.b_build(name, D_L))

    def two_calls():
        op, ex = seqshard_mid.reduce(A, E, True, 1)
        return seqshard_mid.posterior(A, pi, E, op.unsqueeze(2), ex.unsqueeze(2), 0, mode=engine.POST_LOG)

    with options(16):
        torch.cuda.synchronize()
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            eager = [t.clone() for t in two_calls()]           # also the warm-up: the workspace is allocated here
        stream.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(stream):
            with torch.cuda.graph(graph, stream=stream):      # one stream, no branches
                out, ll, phi = two_calls()
        out.fill_(float("nan"))                                # capture does not run the kernels; replay does
        ll.fill_(float("nan"))
        phi.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
    assert torch.equal(out, eager[0]) and torch.equal(ll, eager[1]) and torch.equal(phi, eager[2])


# ---- E: the layer ---------------------------------------------------------------------------------------------------
def test_e_state_posterior_log_probs_sharded_on_a_29_state_cell(monkeypatch):
    """MsaHMMLayer.state_posterior_log_probs_sharded(E_slab, cell) on two slabs, the ranks played in turn through
    seqshard_mid_cases.FakeGroup, against state_posterior_log_probs on the uncut input: sequence 1 carries a run that
    only the floor survives, is flagged, and comes back from gather_flagged as the unsharded call computes it."""
    from hmm_layer_amd import MsaHMMLayer as L5
    from hmm_layer_amd.MsaHmmCell import HmmCell
    from hmm_layer_amd.gene_pred_hmm_emitter import GenePredHMMEmitter
    from hmm_layer_amd.gene_pred_hmm_transitioner import GenePredMultiHMMTransitioner
    codons = dict(start_codons=[("ATG", 1.)], stop_codons=[("TAG", .34), ("TAA", .33), ("TGA", .33)],
                  intron_begin_pattern=[("NGT", .99), ("NGC", .005), ("NAT", .005)],
                  intron_end_pattern=[("AGN", .99), ("ACN", .01)])
    b, L, cut = 3, 400, 170
    g = torch.Generator().manual_seed(29)
    cls = torch.softmax(2 * torch.randn((1, b, L, 15), generator=g), -1)
    nuc = torch.nn.functional.one_hot(torch.randint(0, 5, (1, b, L), generator=g), 5).float()
    x = torch.cat([cls, nuc], -1).to("cuda:0")
    em = GenePredHMMEmitter(**codons, num_copies=2)
    em.build((1, b, L, 15))
    tr = GenePredMultiHMMTransitioner(k=2, initial_exon_len=200, initial_intron_len=4500, initial_ir_len=10000)
    cell = HmmCell([29], 15, em, tr).to("cuda:0")
    A, pi, E0 = L5._engine_inputs(x, cell, None, False)
    assert E0.shape == (1, b, L, 29)
    for hard, no_loglik in ((False, False), (False, True), (True, False), (True, True)):
        mode = engine.POST_LOG_NO_LL if no_loglik else engine.POST_LOG
        E = E0.clone()
        if hard:
            E[0, 1, 150:170] = 0.0                           # the run of the hard cases, ending at the cut
            E[0, 1, 150:170, 8] = 0.5
        want, want_ll = engine.posterior(A, pi, E, mode=mode, eps=cell.epsilon)
        if not hard:                                         # ... which is what the layer's unsharded call returns
            with torch.no_grad():
                assert torch.equal(want, L5._state_posterior_log_probs_impl(x, cell, no_loglik=no_loglik))
        slabs = [E[:, :, :cut].contiguous(), E[:, :, cut:].contiguous()]
        fake = mcs.FakeGroup(slabs)
        fake.install(monkeypatch)
        for r in range(2):                                   # pass 1: what every rank contributes
            fake.play(r, True)
            seqshard.posterior(A, pi, slabs[r], mode=mode)
        flags = ~(sum(fake.reduced[2][r] for r in range(2)) <= seqshard.PHI_LIMIT)
        fake.flag_seqs = flags[0].nonzero().flatten().tolist()
        print("MID-E hard=%s no_loglik=%s flagged %s" % (hard, no_loglik, fake.flag_seqs))
        assert fake.flag_seqs == ([1] if hard else [])
        outs = []
        for r in range(2):                                   # pass 2: the layer call, rank 0 (the root) first
            fake.play(r, False)
            outs.append(L5.state_posterior_log_probs_sharded(slabs[r], cell, no_loglik=no_loglik))
        got = torch.cat([o for o, _ in outs], dim=2)
        assert got.shape == want.shape and got.dtype == torch.float32
        tol = mcs.NO_LL_REL * want_ll.double().abs().max().item() if no_loglik else 0.0

        def gam(t, ll):
            return torch.exp(t.double() - (ll.double()[..., None, None] if no_loglik else 0.0))

        d = (gam(got, outs[0][1]) - gam(want, want_ll)).abs().amax(dim=(0, 2, 3))
        print("MID-E hard=%s no_loglik=%s max |gamma - unsharded| per sequence %s, flagged sequence bit-identical: %s"
              % (hard, no_loglik, d.tolist(), bool(torch.equal(got[0, 1], want[0, 1]))))
        assert float(d.max()) <= 2e-6 + tol                  # the 16-state family's limit against the unsharded call
        for _, ll in outs:
            assert ll.dtype == torch.float64 and ll.shape == (1, b)
            assert ((ll - want_ll.double()).abs() <= mcs.LL_REL * want_ll.double().abs() + mcs.LL_ABS).all()
        assert torch.equal(outs[0][1], outs[1][1])
    with pytest.raises(ValueError, match="64"):
        seqshard.posterior_backend(65)
