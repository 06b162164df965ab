"""Keeps tests/postgrad_small_cases.py honest without a GPU: from the fp64 oracle alone, every case of
tests/test_postgrad_small_gpu.py has finite gradients, few enough columns / rows under the small-scale rule, an fp32
twin far inside the limit under every norm, its clamps engaged in the fp64 recursion and the routing the case is for;
and the table covers the edges it claims, so that a later edit cannot drop one silently."""
import numpy as np
import pytest

import postgrad_small_cases as pc
import postgrad_mid_cases as pm

ALL = pc.all_specs()


@pytest.mark.parametrize("spec", ALL, ids=pc.spec_id)
def test_case_can_carry_the_gpu_comparison(spec):
    c = pc.build(spec)
    k, b, L, q = c["E"].shape
    assert (k, q, b, L) == (len(spec.models), spec.q, spec.b, spec.L)
    assert all(c[n].dtype == np.float32 for n in ("A", "pi", "E", "G"))
    assert k * b * L * q <= 4097 * 64 * 3 and L * q <= 1041 * 16
    if k == 2:
        assert not np.array_equal(c["A"][0], c["A"][1])                 # the models of a call differ
    for m, (ref, rt) in enumerate(zip(pc.reference(spec), pc.routing(spec))):
        name = spec.models[m]
        assert all(np.isfinite(x).all() for x in ref["want"]), m
        rows = c["A"][m].astype(np.float64).sum(-1)
        assert np.all((np.abs(rows - 1) < 1e-5) | ((rows == 0) & (name == "shipped")))
        empty_rows = int((~(c["A"][m] > 0).any(-1)).sum())              # no present edge: nothing for dA/row to hold
        assert empty_rows == (8 if name == "shipped" else 0)
        for n in pc.FINE_NORMS:
            among = q if n != "dE/seq" else b
            exempt = ref["small"][n] * among - (empty_rows if n == "dA/row" else 0)
            assert exempt <= max(1, 0.05 * among) + 1e-9, (m, n, ref["small"][n])
            assert pc.FINE_FACTOR * ref["e32"][n] < pc.FINE_CAP, (m, n, ref["e32"][n])
            assert ref["limit"][n] == max(pc.FINE_FLOOR, pc.FINE_FACTOR * ref["e32"][n])
        assert ref["norms"] == pc.FINE_NORMS                            # fp32 autograd is finite on every case
        skipped = pc.floor_columns(name, c["A"][m])                     # the one exemption is the stated one, and needed
        assert int(skipped.sum()) == (6 if name == "shipped" else 0)
        if name == "shipped":
            assert ref["e32_all_columns"] > 1.0 and not (c["A"][m][:, skipped] > 0).any() and not (c["A"][m][skipped] > 0).any()
        if q == 1:                                                      # gamma = 1: the gradient vanishes identically
            assert all(np.all(x == 0.0) for x in ref["want"])
            assert max(ref["absolute"]) < pc.Q1_OF_G * np.abs(c["G"][m]).max()
            assert min(ref["absolute"]) >= pc.Q1_ABS
        else:
            assert ref["absolute"] is None
            assert ref["e32"]["tensor"] <= pc.TENSOR_REL / pc.FINE_FACTOR
        gam, count = pm.forward_backward64(c["A"][m], c["pi"][m], c["E"][m])
        assert count == rt["count"]
        assert np.abs(gam.sum(-1) - 1).max() <= 1e-12
        for clamp in pc.engages(spec)[m]:
            assert count[clamp] >= 1, (m, clamp, count)
        if spec.G == "label":                                           # one label per position, on its most probable state
            assert np.array_equal(c["G"][m], -(gam == gam.max(-1, keepdims=True)).astype(np.float32))
            assert np.all(c["G"][m].sum(-1) == -1.0)
            if spec.log:                                                # nothing of the weight on a negligible state
                assert gam[c["G"][m] < 0].min() > 1.0 / (2 * q)
    if pc.forced_per_chunk(spec):
        assert pc.unclamped(spec) and pc.chunks(spec) >= 2


def test_routing_predictions():
    """The cases that are there for the per-chunk path are predicted to take it, sequence by sequence."""
    def verdicts(s):
        return [(s.models[m], v) for m, r in enumerate(pc.routing(s)) for v in r["verdict"]]
    per_chunk = pc.geometry_sweep() + pc.fold_cases() + [s for s in pc.clamp_cases() if not s.log and s.emis == "clamp"] \
        + pc.warmup_cases()
    for s in per_chunk:
        for name, v in verdicts(s):
            # (fclamp: its 1e-20 edge is below eps, so nothing enters state D in the support k_topo_check reads and the
            # model goes to the whole-sequence sweeps as a model; fclamp2 is the forward clamp the per-chunk path serves)
            assert v == ("whole" if name in ("triu", "fclamp") else "chunk"), (pc.spec_id(s), name, v)
    for s in pc.two_model_cases():
        assert verdicts(s) == [("gene", "chunk")] * s.b + [("shipped", "whole")] * s.b
    for s in pc.clamp_cases() + [s for s in pc.warmup_cases() if s.emis == "clamp"]:
        r = pc.routing(s)[0]
        assert r["primitive"] == (s.models[0] != "fclamp")
        if s.emis == "stretch":
            seq = pc.STRETCH[0]
            assert r["verdict"] == ["whole" if i == seq else "chunk" for i in range(s.b)]
            assert r["F"][seq] > 1e3 * pc.EXACT_DELTA
        elif s.models[0] != "bclamp":                                   # the clamp at (nearly) every position of every sequence
            assert r["count"]["forward"] >= 0.99 * s.b * (s.L - 1)
            if s.models[0] == "fclamp2":                                # in the support by a quarter of eps
                assert pc.build(s)["A"][0, 0, s.q - 1] == np.float32(pc.FCLAMP2_EDGE) > np.float32(1.2 * pc.EPS)
        else:
            assert r["count"]["backward"] >= 0.5 * s.b * (s.L - 1)
    for s in ALL:                                                        # the bounds the GPU test holds the count to
        lo, hi = pc.serial_bounds(s)
        assert 0 <= lo <= hi <= len(s.models) * s.b
        if not pc.shipped_per_chunk(s):
            assert lo == hi == len(s.models) * s.b


def test_the_sweep_covers_what_it_is_for():
    assert len({pc.spec_id(s) for s in ALL}) == len(ALL)
    assert set(pc.SEEDS) <= {pc.spec_id(s) for s in ALL}                 # no stale entry in the table of replaced seeds
    assert pc.SWEEP_L % 8 == 3 and pc.SWEEP_L // 8 == 25                # MQ_PF = 8: whole blocks and a tail
    assert all(s.G == "label" for s in ALL if s.log and s.emis in ("rare", "dead"))
    for log in pc.MODES:
        mine = [s for s in ALL if s.log == log]
        sweep = [s for s in pc.state_sweep() if s.log == log]
        assert all((s.b, s.L, s.T) == (pc.SWEEP_B, pc.SWEEP_L, 0) and pc.shipped_per_chunk(s) == (s.q > 1) for s in sweep)
        prim = [s for s in sweep if s.models[0] in ("dense", "sparse")]
        assert sorted(s.q for s in prim) == list(range(1, 17))          # every q, on a model the per-chunk path may serve
        assert all(pc.routing(s)[0]["primitive"] for s in prim)
        assert [s.models[0] for s in sorted(prim, key=lambda s: s.q)] == ["sparse", "dense"] * 8
        assert {s.q for s in sweep if s.models[0].endswith("-d")} == set(range(4, 17))
        for name, q in (("gene", 15), ("simple7", 7)):
            assert {(s.emis, s.G) for s in sweep if s.models == (name,)} == \
                {("holes", "dense"), ("rare", "label"), ("dead", "label")}
        assert {(s.q, s.L) for s in pc.length_sweep() if s.log == log} == {(q, L) for q in (5, 15, 16) for L in pc.LENGTHS}
        assert all(len(s.models) == 2 for s in pc.length_sweep() + pc.batch_sweep())
        # chunk geometry: C and the last chunk's length at T = 16, the warm-up at every T
        geo = [s for s in pc.geometry_sweep() if s.log == log]
        for name, q in pc.GEOMETRY_MODELS:
            g = [s for s in geo if s.models == (name,) and s.q == q]
            assert all(s.b == 2 and pc.chunk_len(s) == s.T for s in g)
            t16 = sorted((s for s in g if s.T == 16), key=lambda s: s.L)
            assert [pc.chunks(s) for s in t16] == [2, 3, 3, 4, 4, 5, 5, 5, 5, 9, 66]
            assert {pc.last_chunk(s) for s in t16} >= {1, 2, 15, 16}
            assert {s.L % 64 > 48 or s.L % 64 == 0 for s in t16} == {False, True}     # waves with and without idle rows
            assert max(pc.chunks(s) for s in t16) > 64                  # the c += 64 strides of k_pc_scan and k_pc_fold
            assert {(s.T, s.L, pc.warmup_chunks(s)) for s in g if s.T != 16} == {(48, 193, 2), (64, 257, 1), (80, 321, 1)}
            assert all(pc.warmup_chunks(s) == 4 for s in t16)
            # the warm-up is clipped at both ends (fewer chunks than it wants on either side) and unclipped inside
            assert any(pc.chunks(s) > 2 * pc.warmup_chunks(s) for s in g) and any(pc.chunks(s) <= pc.warmup_chunks(s) for s in g)
        # both sides of both boundaries of pc_wanted, through the shipped routing
        assert {pc.chunks(s) for s in geo} >= {pc.PC_MIN_CHUNKS - 1, pc.PC_MIN_CHUNKS}
        nb = {len(s.models) * s.b for s in pc.fold_cases() if s.log == log}
        assert nb >= {pc.PC_MAX_SEQS, pc.PC_MAX_SEQS + 1}
        assert [pc.shipped_per_chunk(s) for s in pc.fold_cases() if s.log == log and s.q == 3] == [True, False]
        # both fold kernels; a reducible model beside a per-chunk one above the threshold (C = 4: a wave per sequence,
        # so these waves do not straddle the models; the 39-chain case below does)
        assert nb >= {pc.PC_FOLD_WAVES_MAX_SEQS, pc.PC_FOLD_WAVES_MAX_SEQS + 1}
        assert all(pc.chunks(s) == 4 and pc.shipped_per_chunk(s) for s in pc.fold_cases() if s.log == log and s.q == 5)
        mixed = [s for s in pc.fold_cases() if s.log == log and s.models == ("dense", "triu")]
        assert len(mixed) == 1 and mixed[0].b == 129
        assert {s.b for s in pc.batch_sweep() if s.log == log} == {1, 64, 65, 130}
        assert all(not pc.shipped_per_chunk(s) for s in pc.batch_sweep() + pc.length_sweep())
        two = [s for s in pc.two_model_cases() if s.log == log]
        assert len(two) == 1 and two[0].b * pc.chunks(two[0]) == 39 and 39 % 4 != 0
        assert {(s.q, s.models[0]) for s in pc.clamp_cases() if s.log == log and s.emis == "clamp"} == \
            {(q, n) for q in (6, 16) for n in ("fclamp", "fclamp2", "bclamp")}
        assert all((s.b, s.L, s.T) == (3, 130, 16) for s in pc.clamp_cases() if s.emis == "clamp")
        # the runs without a certificate include two and three chunks
        assert {2, 3} <= {pc.chunks(s) for s in mine if pc.forced_per_chunk(s)}
    assert [s.log for s in pc.clamp_cases() if s.emis == "stretch"] == [False, True]
    # the warm-up of a single chunk (a warm-up one chunk late is none), on the clamp constructions and rare / dead emissions
    w = pc.warmup_cases()
    assert all(pc.warmup_chunks(s) == 1 and pc.chunks(s) == 5 and pc.shipped_per_chunk(s) for s in w)
    assert {(s.models[0], s.emis, s.log) for s in w} >= {(n, e, log) for log in pc.MODES for n, e in
                                                         (("fclamp2", "clamp"), ("bclamp", "clamp"), ("gene", "rare"), ("gene", "dead"))}
    # the PGCHUNK = 2 runs are decided by the fp64 recursion itself, for every case
    for s in ALL:
        assert pc.forced_per_chunk(s) == (s.q > 1 and pc.chunks(s) >= 2 and pc.unclamped(s)
                                          and all(r["primitive"] for r in pc.routing(s)))


def test_chunk_length_rule():
    """pc.chunk_len restates pc_chunk_len / choose_T for the unforced cases: values read off the engine's rule."""
    S = lambda b, L, T=0, k=1: pc.Spec(("dense",) * k, 5, b, L, "plain", "dense", False, 0, T)
    assert [pc.chunk_len(S(3, L)) for L in (1, 16, 17, 24, 203, 9999)] == [16, 16, 16, 16, 16, 96]
    assert pc.chunk_len(S(32, 9999)) == 96 and pc.chunk_len(S(2, 100000)) == 272
    assert pc.chunk_len(S(3, 203, 48)) == 48
    assert (pc.chunks(S(2, 1041, 16)), pc.last_chunk(S(2, 1041, 16))) == (66, 1)


def test_build_is_deterministic_and_read_only():
    s = pc.state_sweep()[1]
    a = pc.build(s)
    pc._build.cache_clear()
    b = pc.build(s)
    assert a is not b and all(np.array_equal(a[n], b[n]) for n in a)
    with pytest.raises(ValueError):
        a["E"][0, 0, 0, 0] = 1.0
    with pytest.raises(ValueError):
        pc.reference(s)[0]["want"][2][0, 0, 0] = 1.0
    with pytest.raises(ValueError):
        pc.fixed_model("shipped")[0][0, 0] = 1.0


def test_absent_edges_are_split_off_for_per_chunk_runs_only():
    rng = np.random.default_rng(0)
    A = np.asarray(pm.rand_model(rng, 9, sparse=True)[0])
    want = (rng.standard_normal((9, 9)), rng.standard_normal(9), rng.standard_normal((2, 5, 9)))
    got = [x.copy() for x in want]
    i, j = np.argwhere(A == 0)[0]
    got[0][i, j] += 1e-2 * np.abs(want[0]).max()
    whole, _ = pc.errors(got, want, A, False)
    chunk, _ = pc.errors(got, want, A, True)
    assert whole["tensor"] > pc.TENSOR_REL and chunk["tensor"] <= 0 and chunk["dA/row"] == whole["dA/row"] == 0
    assert abs(whole["dA/absent"] - 1e-2) < 1e-12 and chunk["dA/absent"] == whole["dA/absent"] < pc.ABSENT_REL
