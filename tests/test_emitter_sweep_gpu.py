"""hmm_gene_emissions (1..64 states: k_gene_emissions<1,1,FAST>, <1,1,false>, <4,2,false>) and hmm_gene_emissions_wide
(1..256 states) against the fp64 loop reference of tests/emitter_cases.py.  Needs an MI355X.

Cases, reference and tolerance: tests/emitter_cases.py; tests/test_emitter_sweep_cpu.py shows without a device that the
reference is the definition (against the kmer-based restatement and the recorded outputs of the original project), that
every case can carry the comparison, that every instantiation is reached, and that the case set notices eight wrong
readings of the definition.  Per element |got - want| <= (s + 140) 2^-24 want, and got == 0 exactly where want == 0.
  (a) table sweep: every q x s of either kernel with rows in {1, 7, 32} / {1, 33, 256}, nc in {0, 1, 9, 16} /
      {0, 9, 16}, both (add, n_mass) settings, state_row and state_codon entries out of range;
  (b) position sweep: every L from 1 to 40, the soft mixture at eleven lengths, six shapes around the run edges;
  (c) soft placement: one irregular row per sequence at every tile position;
  (d) run-loop wrap: 8 454 200 positions, past the 8 388 608 that one round of the grid's waves covers.
Repeated calls are bit-identical, and so are the two kernels on every narrow case of (a) and (b) (q <= 64, rows <= 32).
Every item prints its worst err / bound (pytest -s) before it asserts.

Measured on an MI355X (worst err / bound per family and kernel; every figure is printed by the tests):
    (a) <1,1,FAST> 0.038   <1,1,false> 0.039   <4,2,false> 0.054   wide 0.046
    (b) every L from 1 to 40:  q15 (FAST) 0.049   q7 (<1,1,false>) 0.047   q29 (<4,2,false>) 0.066   q71 (wide) 0.052
        the soft mixture:      q15 0.040   q7 0.051   q29 0.049   q71 0.059
        the run edges:         q15 0.049   q7 0.049   q29 0.057   q71 0.050
    (c) q15 0.047   q7 0.041   q29 0.056   q71 0.049; the windows that see the irregular row at most 0.038, the
        others at most 0.056
    (d) narrow 0.032: the call 0.004 s, the comparison 0.43 s (9 blocks; the item runs first and pays the first use
        of torch's comparison kernels), the second call with its comparison 0.004 s; wide 0.039: the call 0.029 s, the
        comparison 0.023 s (65 blocks of 34 MB, about 0.5 GB of traffic each), the second call with its comparison
        0.030 s.  Both items stay: the slower takes 0.5 s, the slowest of the file
Every zero of the reference came out as an exact zero; the two kernels agreed bit for bit on all 132 + 171 cases; the
whole file ran in 5 s, twice with the same figures.  The sweep found no defect: the kernels sit at about a twentieth of the derived bound, the level
of the fp32 twin (0.06 at most).
"""
import time

import numpy as np
import pytest
import torch

import emitter_cases as ec
from hmm_layer_amd import engine

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INSTANTIATIONS = ("<1,1,FAST>", "<1,1,false>", "<4,2,false>", "wide")
NARROW_SETS = [name for name, t in ec.TABLE_SETS.items() if not t[4]]


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)            # (a copy: the cases are read-only)


def run(spec, wide, x=None):
    c = ec.build(spec)
    fn = engine.gene_emissions_wide if wide else engine.gene_emissions
    return fn(dev(c["x"]) if x is None else x, dev(c["B"]), dev(c["row"]), dev(c["codon"]), dev(c["cod"]),
              free_value=spec.free, add=spec.add, n_mass=spec.n_mass)


def sweep(tag, cases, wide=None):
    """Every case through its kernel against the reference -> the failures; prints the worst err / bound."""
    failed, worst, at = [], 0.0, None
    for spec in cases:
        got = run(spec, spec.wide if wide is None else wide).cpu().numpy()
        assert got.shape == (spec.b, spec.L, spec.q)
        err, zeros = ec.compare(got, ec.reference(spec), spec.s)
        if err > worst:
            worst, at = err, spec
        if not (np.isfinite(got).all() and err <= 1.0 and zeros == 0):
            print("SWEEP FAILED %s: err / bound %.3g, %d zeros differ" % (ec.spec_id(spec), err, zeros))
            failed.append(ec.spec_id(spec))
    print("SWEEP %s: %d cases, worst err / bound %.3f (%s)" % (tag, len(cases), worst, at and ec.spec_id(at)))
    return failed


@pytest.mark.parametrize("inst", INSTANTIATIONS)
def test_table_sweep(inst):
    cases = [c for c in ec.all_cases("a") if ec.instantiation(c.q, c.s, c.wide) == inst]
    assert len(cases) >= 10
    assert not sweep("(a) %s" % inst, cases)


@pytest.mark.parametrize("block", ec.POSITION_BLOCKS)
@pytest.mark.parametrize("name", list(ec.TABLE_SETS))
def test_position_sweep(name, block):
    assert not sweep("(b) %s %s" % (name, block), ec.position_cases(name, block))


@pytest.mark.parametrize("name", list(ec.TABLE_SETS))
def test_soft_placement(name):
    """One irregular row per sequence, at position 12 + i: the five positions whose windows see it, and every other."""
    failed, worst = [], 0.0
    for spec in ec.placement_cases(name):
        got, want = run(spec, spec.wide).cpu().numpy(), ec.reference(spec)
        assert got.shape == want.shape and np.isfinite(got).all()
        near = np.zeros((spec.b, spec.L), bool)
        for i in range(spec.b):
            near[i, 10 + i:15 + i] = True
        err_near, z_near = ec.compare(got[near], want[near], spec.s)
        err_far, z_far = ec.compare(got[~near], want[~near], spec.s)
        print("SWEEP (c) %s %s: windows that see the irregular row %.3f, the others %.3f" % (name, spec.nuc, err_near, err_far))
        worst = max(worst, err_near, err_far)
        if z_near or z_far or err_near > 1.0 or err_far > 1.0:
            failed.append((ec.spec_id(spec), err_near, z_near, err_far, z_far))
    print("SWEEP (c) %s: worst err / bound %.3f" % (name, worst))
    assert not failed


@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
def test_run_loop_wrap(wide):
    """One sequence of 1031 positions repeated 8200 times on the device: the runs above number 8192 are served by the
    run loop's second round.  Every sequence equals the first bit for bit, the first meets the reference, and a second
    call gives the same bits.  The times are wall-clock around device synchronisations; every block's comparison ends
    in a host read, so they include the waits."""
    spec = ec.WRAP[wide]
    b, L, q = ec.WRAP_B, spec.L, spec.q
    assert b * L > ec.WRAP_POSITIONS
    want = dev(ec.reference(spec)[0])                                       # (L, q) fp64
    x = dev(ec.build(spec)["x"]).expand(b, L, spec.s + 5).contiguous()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    E = run(spec, wide, x=x)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    assert E.shape == (b, L, q)
    nz = want != 0
    lim = ec.bound(spec.s) * want
    worst, same, zeros_ok = 0.0, True, True
    step = 128 if wide else 1024
    for i in range(0, b, step):
        blk = E[i:i + step]
        same = same and bool((blk == E[0]).all())
        d = (blk.double() - want).abs()
        worst = max(worst, float((d[:, nz] / lim[nz]).max()))
        zeros_ok = zeros_ok and bool(((blk == 0) == ~nz).all())
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    again = run(spec, wide, x=x)                                            # family (d)'s repeated call
    repeat = torch.equal(again, E)
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    print("SWEEP (d) %s: %d positions, worst err / bound %.3f; the call %.3f s, the comparison %.3f s, the second call "
          "and its comparison %.3f s" % ("wide" if wide else "narrow", b * L, worst, t1 - t0, t2 - t1, t3 - t2))
    assert same and zeros_ok and repeat and worst <= 1.0


def test_repeated_calls_are_bit_identical():
    """A case of (a), (b) and (c) through each kernel; (d)'s repeated call is in test_run_loop_wrap."""
    for spec in (ec.table_cases(False)[40], ec.table_cases(True)[40], ec.position_cases("q29", "edges")[4],
                 ec.position_cases("q71w", "soft")[-1], ec.placement_cases("q15")[1], ec.placement_cases("q71w")[0]):
        first = run(spec, spec.wide)
        for _ in range(2):
            assert torch.equal(run(spec, spec.wide), first), ec.spec_id(spec)


def test_both_kernels_give_the_same_bits_on_the_table_sweep():
    """Every narrow case of (a) is a shape both kernels serve (q <= 64, rows <= 32)."""
    for spec in ec.table_cases(False):
        assert ec.serves(spec, True) and ec.serves(spec, False)
        assert torch.equal(run(spec, True), run(spec, False)), ec.spec_id(spec)


@pytest.mark.parametrize("name", NARROW_SETS)
def test_both_kernels_give_the_same_bits_on_the_position_sweep(name):
    for block in ec.POSITION_BLOCKS:
        for spec in ec.position_cases(name, block):
            assert ec.serves(spec, True) and ec.serves(spec, False)
            assert torch.equal(run(spec, True), run(spec, False)), ec.spec_id(spec)
