"""The sweep of the gene-emitter forwards, without a device: the loop reference of tests/emitter_cases.py against the
kmer-based restatement and against the reference's recorded outputs, the validity and the reach of the cases, their
sensitivity to eight wrong readings of the definition, and the argument checks of the two entry points."""
import ctypes

import numpy as np
import pytest
import torch

import emitter_cases as ec
from hmm_layer_amd import build as hbuild
from hmm_layer_amd import engine
from hmm_layer_amd.gene_pred_hmm_emitter import GenePredHMMEmitter
from oracle import params

OK, BAD_SHAPE, Q_UNSUPPORTED, NULL_POINTER, WORKSPACE = 0, -1, -2, -3, -4
CODONS = dict(start_codons=[("ATG", 1.)], stop_codons=[("TAG", .34), ("TAA", .33), ("TGA", .33)],
              intron_begin_pattern=[("NGT", .99), ("NGC", .005), ("NAT", .005)],
              intron_end_pattern=[("AGN", .99), ("ACN", .01)])
INSTANTIATIONS = ("<1,1,FAST>", "<1,1,false>", "<4,2,false>", "wide")
FAMILIES = "abc"


@pytest.mark.parametrize("fam", FAMILIES)
def test_loop_reference_equals_the_kmer_restatement(fam):
    worst = 0.0
    for spec in ec.all_cases(fam):
        want, other = ec.reference(spec), ec.restatement(spec)
        assert want.shape == other.shape == (spec.b, spec.L, spec.q)
        assert np.array_equal(want == 0, other == 0), ec.spec_id(spec)
        nz = want != 0
        rel = float((np.abs(other - want)[nz] / want[nz]).max())
        worst = max(worst, rel)
        assert rel <= 1e-12, (ec.spec_id(spec), rel)
    print("family (%s): %d cases, loop against restatement %.3g relative" % (fam, len(ec.all_cases(fam)), worst))


def golden_variants(golden):
    """(tag, x, kernel, copies, shared, training, d5_compat, the recorded E) of both fixture files."""
    z = golden("emitter")
    x = torch.from_numpy(z["x"])
    yield "c1", x, z["kernel"], 1, True, False, False, z["E"]
    yield "c1 d5_compat", x, z["kernel"], 1, True, False, True, z["E_as_shipped"]
    yield "c1 training", x, z["kernel"], 1, True, True, False, z["E_training"]
    yield "c2 unshared", x, z["kernel_c2"], 2, False, False, False, z["E_c2"]
    z = golden("emitter_wide")
    x = torch.from_numpy(z["x"])
    for c, shared in z["models"]:
        tag = "c%d_%s" % (int(c), "shared" if shared else "unshared")
        for training in (False, True):
            yield (tag + " training" * training, x, z[tag + "_kernel"], int(c), bool(shared), training, True,
                   z[tag + ("_E_training" if training else "_E")])


def test_loop_reference_equals_the_recorded_outputs(golden):
    """The gene models' own tables (the emitter's state_tables and codon_probs, B = softmax of the recorded kernel)
    through the loop reference against oracle.params.gene_emissions, which is the recorded output of the original
    project bit for bit.  Those are fp32 evaluations, so the comparison is the sweep's own: the relative bound, zeros
    exact."""
    tab = params.codon_table(**params.DEFAULT_CODONS)
    for tag, x, kernel, copies, shared, training, d5, recorded in golden_variants(golden):
        em = GenePredHMMEmitter(**CODONS, num_copies=copies, share_intron_parameters=shared)
        em.build((1,) + tuple(x.shape[1:3]) + (15,))
        row, cod = em.state_tables(torch.device("cpu"))
        B = torch.softmax(torch.as_tensor(kernel[0], dtype=torch.float32), -1).numpy()
        assert B.shape[0] == em.kernel_rows() and row.numel() == recorded.shape[-1]
        oracle = params.gene_emissions(x, kernel, tab, copies=copies, share_intron=shared, training=training,
                                       d5_compat=d5).numpy()
        assert np.array_equal(oracle, recorded), tag
        want = ec.reference_arrays(x[0].numpy(), B, row.numpy(), em.codon_probs.numpy(), cod.numpy(), 1.0 / 4096.0,
                                   1e-7 if training else 0.0, 2 if d5 else 1)
        worst, zeros = ec.compare(oracle[0], want, 15)
        print("%s: recorded output at %.3g of the bound, %.0f %% zeros" % (tag, worst, 100 * (want == 0).mean()))
        assert zeros == 0 and worst <= 1.0, (tag, worst, zeros)


@pytest.mark.parametrize("fam", FAMILIES + "d")
def test_every_case_can_carry_the_comparison(fam):
    smallest, zeros, twin = 1.0, 0.0, 0.0
    for spec in ec.all_cases(fam):
        assert ec.violations(spec) == [], ec.spec_id(spec)
        want = ec.reference(spec)
        smallest, zeros = min(smallest, want[want != 0].min()), max(zeros, (want == 0).mean())
        twin = max(twin, ec.compare(ec.restatement(spec, fp32=True), want, spec.s)[0])
    print("family (%s): smallest non-zero %.3g, at most %.0f %% zeros, fp32 twin at most %.3g of the bound"
          % (fam, smallest, 100 * zeros, twin))


def test_every_instantiation_is_reached():
    count = {}
    for spec in ec.all_cases("a"):
        assert ec.serves(spec, spec.wide), ec.spec_id(spec)
        count[ec.instantiation(spec.q, spec.s, spec.wide)] = count.get(ec.instantiation(spec.q, spec.s, spec.wide), 0) + 1
    print("cases of (a) per instantiation:", count)
    assert set(count) == set(INSTANTIATIONS) and min(count.values()) >= 10
    # the four table sets of (b) and (c) are one per instantiation, and each runs every shape of the two families
    sets = {name: ec.instantiation(q, s, wide) for name, (q, s, rows, nc, wide) in ec.TABLE_SETS.items()}
    assert sorted(sets.values()) == sorted(INSTANTIATIONS)
    shapes = {name: [(c.b, c.L, c.nuc) for block in ec.POSITION_BLOCKS for c in ec.position_cases(name, block)]
              + [(c.b, c.L, c.nuc) for c in ec.placement_cases(name)] for name in ec.TABLE_SETS}
    assert all(v == shapes["q15"] for v in shapes.values())
    assert [(5, L, "hot") for L in range(1, 41)] + [(5, L, "soft") for L in ec.SOFT_L] \
        + [(b, L, "hot") for b, L in ec.RUN_EDGES] + [(24, 64, "place"), (24, 64, "placeN")] == shapes["q15"]
    for name in ec.TABLE_SETS:
        for c in [c for block in ec.POSITION_BLOCKS for c in ec.position_cases(name, block)] + list(ec.placement_cases(name)):
            assert ec.instantiation(c.q, c.s, c.wide) == sets[name] and ec.serves(c, c.wide)


def test_the_table_sweep_meets_every_value():
    """(a): every q and every s of either kernel meets every rows, every nc and both (add, n_mass) settings; the
    out-of-range entries reach every instantiation; the wrap cases cross the run loop's stride."""
    for wide, Q, S, R, NC in ((False, ec.NARROW_Q, ec.NARROW_S, ec.NARROW_ROWS, ec.NARROW_NC),
                              (True, ec.WIDE_Q, ec.WIDE_S, ec.WIDE_ROWS, ec.WIDE_NC)):
        cases = ec.table_cases(wide)
        assert {(c.q, c.s) for c in cases} == {(q, s) for q in Q for s in S} and len(cases) == len(Q) * len(S)
        for q in Q:
            mine = [c for c in cases if c.q == q]
            assert {c.rows for c in mine} == set(R) and {c.nc for c in mine} == set(NC), q
            assert {(c.add, c.n_mass) for c in mine} == set(ec.SETTINGS) and {c.free for c in mine} == set(ec.FREE), q
        for i in range(0, len(cases), 3):
            assert cases[i].bad in (1, 2, 3) and cases[i + 1].bad == 4 and cases[i + 2].bad == 0
    for inst in INSTANTIATIONS:
        mine = [c for c in ec.all_cases("a") if ec.instantiation(c.q, c.s, c.wide) == inst]
        assert {1, 2, 3, 4} <= {c.bad for c in mine}, inst
        # an entry out of range changes the value it would otherwise have
        for c in mine:
            t = ec.tables(c.q, c.s, c.rows, c.nc, c.tset, c.bad)
            if 1 <= c.bad <= 3:
                assert ((t["row"] < 0) | (t["row"] >= c.rows)).any()
            elif c.bad == 4:
                assert (t["cod"] == c.nc + 3).any() and (c.q == 1 or (t["cod"] == -5).any())
    for spec in ec.WRAP.values():
        assert ec.WRAP_B * spec.L >= ec.WRAP_POSITIONS + 64 * ec.EM_RUN        # 64 runs and more take the stride
        assert (ec.tables(spec.q, spec.s, spec.rows, spec.nc, spec.tset)["cod"] >= 0).any()


def test_the_position_sweep_holds_the_tiles_the_kernel_branches_on():
    """From (P mod L, L) alone: fast-path tiles at both ends of the predicate tb >= 2 && tb + 18 <= L, tiles that miss
    either condition by one, tiles of three and more sequences, the run edges."""
    seen = dict(tb2=0, end=0, tb1=0, end1=0, three=0, ragged=0)
    for spec in ec.position_cases("q15", "L1-40"):
        npos = spec.b * spec.L
        for P, tb in ec.tiles(spec):
            fast = ec.fast_tile(P, tb, spec.L, npos)
            seen["tb2"] += fast and tb == 2
            seen["end"] += fast and tb + 18 == spec.L
            seen["tb1"] += tb == 1 and tb + 18 <= spec.L and P + 16 <= npos
            seen["end1"] += tb >= 2 and tb + 18 == spec.L + 1 and P + 16 <= npos
            seen["three"] += ec.sequences_in_tile(P, spec.L, npos) >= 3
            seen["ragged"] += P + 16 > npos
    print("tiles of the position sweep:", seen)
    assert all(v > 0 for v in seen.values()), seen
    run = ec.EM_RUN
    edges = {(c.b, c.L) for c in ec.position_cases("q15", "edges")}
    assert (2, 1024) in edges                                             # a run boundary on a sequence boundary
    assert (2, 1023) in edges and (2, 1025) in edges                      # one position either side of it
    b, L = 1, 2050                                                        # a boundary inside a sequence, on the fast path
    assert (b, L) in edges and ec.fast_tile(run, run % L, L, b * L) and ec.fast_tile(run - 16, (run - 16) % L, L, b * L)
    assert (9, 1000) in edges and 9 * 1000 > 8 * run                      # a ninth run: a second workgroup
    assert (1, 8300) in edges and 8300 > 8 * run                          # ... inside one sequence
    # (c): the irregular rows lie at tile positions 12..15, 0..15 and 0..3 of three tiles
    at = [12 + i for i in range(24)]
    assert {t % 16 for t in at} == set(range(16)) and {t // 16 for t in at} == {0, 1, 2}
    for spec in ec.placement_cases("q15"):
        x = ec.build(spec)["x"][..., spec.s:]
        hot = ((x[..., :4] == 1).sum(-1) == 1) & (x[..., :4].sum(-1) == 1) & (x[..., 4] == 0)
        exact_n = (x[..., :4] == 0).all(-1) & (x[..., 4] == 1)
        odd = ~(hot | exact_n)
        assert np.array_equal(np.argwhere(odd), np.array([(i, 12 + i) for i in range(24)])), spec.nuc


@pytest.mark.parametrize("variant", list(ec.VARIANTS))
def test_a_wrong_reading_of_the_definition_is_noticed(variant):
    """At least one case of the named family differs from the reference by more than ten times the bound."""
    fam = ec.VARIANTS[variant]
    caught, worst = 0, 0.0
    for spec in ec.all_cases(fam):
        want, wrong = ec.reference(spec), ec.restatement(spec, variant=variant)
        nz = want != 0
        ratio = float((np.abs(wrong - want)[nz] / (ec.bound(spec.s) * want[nz])).max())
        hit = ratio > 10 or bool((wrong[~nz] != 0).any())
        caught, worst = caught + hit, max(worst, ratio)
    print("%s: %d of %d cases of (%s) differ by more than 10 bounds; the largest by %.3g" % (
        variant, caught, len(ec.all_cases(fam)), fam, worst))
    assert caught >= 1


# ------------------------------------------------------------------------------------------------ the argument check

@pytest.fixture(scope="module")
def lib():
    hbuild.build()
    return engine.lib()


F = ctypes.c_float


def fwd(lib, name, b=2, L=3, s=15, rows=13, nc=9, q=15, ptrs=(256,) * 6):
    """The forward with placeholder device pointers: every call here returns before any HIP call."""
    x, B, state_row, codon, state_codon, E = ptrs
    return getattr(lib, name)(x, b, L, s, B, rows, state_row, codon, nc, state_codon, q, F(1.0 / 4096), F(0.0), 1, E, None)


def test_documented_codes_of_the_argument_check(lib):
    narrow, wide = "hmm_gene_emissions", "hmm_gene_emissions_wide"
    for name in (narrow, wide):
        assert fwd(lib, name, nc=17) == Q_UNSUPPORTED
        assert fwd(lib, name, s=33) == Q_UNSUPPORTED
        assert fwd(lib, name, nc=-1) == BAD_SHAPE
        assert fwd(lib, name, nc=9, ptrs=(256, 256, 256, None, 256, 256)) == NULL_POINTER      # tables without codon
    assert fwd(lib, narrow, q=65) == Q_UNSUPPORTED and fwd(lib, narrow, q=64, ptrs=(None,) * 6) == NULL_POINTER
    assert fwd(lib, narrow, rows=33) == Q_UNSUPPORTED
    assert fwd(lib, wide, q=257) == Q_UNSUPPORTED and fwd(lib, wide, q=256, rows=256, ptrs=(None,) * 6) == NULL_POINTER
    # nc = 0 with codon NULL: a forward call that the check accepts would launch, so the evidence without a device is
    # the backward entry points.  They share the check (em_check_args) and have one more behind it: with nc = 0 they
    # get past the pointers and stop at the workspace, with nc = 9 the same call stops at the NULL codon.  The device
    # sweep runs the forwards with nc = 0.
    for name in ("hmm_gene_emissions_grad", "hmm_gene_emissions_grad_wide"):
        args = (256, 2, 3, 15, 256, 13, 256, None, 0, 256, 15, F(1.0 / 4096), F(1e-7), 1, 256, 256, 256, 256, 0, None)
        assert getattr(lib, name)(*args) == WORKSPACE
        assert getattr(lib, name)(*(args[:7] + (None, 9) + args[9:])) == NULL_POINTER
