"""Inputs, the fp64 reference and the limits of the sweep of the gene-emitter forwards, hmm_gene_emissions (1..64
states) and hmm_gene_emissions_wide (1..256), tests/test_emitter_sweep_cpu.py and tests/test_emitter_sweep_gpu.py.

Test infrastructure; imports neither the engine nor a GPU.

reference(spec) is the definition of include/hmm_engine.h and of the header comment of csrc/hmm_emitter.inc in fp64
numpy, with an explicit loop over the positions and the states vectorised; it does not use hmm_layer_amd/kmer.py.  Per
position: three slot distributions per side (positions t, t+1, t+2 on the left, t, t-1, t-2 on the right; a slot outside
the sequence is uniform 1/4; an N flag that is exactly 1 adds 1/4 to each base on the left and n_mass/4 on the right),
the 64 products of each side at the indices 16 n(t+1) + 4 n(t+2) + n(t) and 16 n(t-1) + 4 n(t-2) + n(t), their sums
against the state's two table rows, and E = emit (factor + add).  state_row is clamped to 0..rows-1; state_codon < 0 is a
free state (factor = free_value), state_codon >= nc reads row nc - 1, nc = 0 makes every state free.

restatement(spec, dtype, variant) is the kmer-based restatement of tests/test_emitter_wide_gpu.py (with the table rules
above).  In fp64 it checks the loop, in fp32 it is the reference's twin (the error an fp32 evaluation of the same
definition makes), and its deliberately wrong variants (VARIANTS) show that the case set tells them apart.

A case is a Spec:
  fam     "a" table sweep, "b" position sweep, "c" soft placement, "d" run-loop wrap
  q, s, rows, nc, tset   the tables (tables()): B = softmax(randn) (rows, s); state_row uniform; codon (2, nc, 64)
          uniform with half the entries exactly 0; state_codon free (-1) with probability 0.4, else a uniform row
  bad     0; 1..3: two entries of state_row out of range (two of -7, rows, 1 << 20); 4: state_codon holds -5 and nc + 3
  b, L, nuc   the input (inputs()): class columns softmax(2 randn); nucleotides
          "hot"     one-hot with 20 % N
          "soft"    the mixture of the existing emitter tests on top: 15 % soft rows, 5 % N flag 0.5, 5 % N = 1 next to
                    a base
          "place"   one-hot without N; sequence i has one irregular row at position 12 + i, its kind i mod 5: a soft
                    row, N flag 0.5, N = 1 next to a base, an all-zero row, (0.5, 0.5, 0, 0, 0)
          "placeN"  the same on one-hot with 20 % N
  add, n_mass, free   the three scalars of the call
  wide    the case is meant for hmm_gene_emissions_wide (the narrow cases of (a) and (b) run through both where both
          serve the shape)

Tolerance.  Every term of every sum is non-negative, so the relative error of the fp32 result is bounded by the number
of roundings on its path: s for the class sum, 64 + 3 per side for the product-sum (or the table entry with its N
weights), a handful for the products and `+ add`: |got - want| <= (s + 140) 2^-24 want per element (1.03e-5 at s = 32,
inside the project's 2e-5), and got == 0 exactly where want == 0.

violations(spec): the reference is finite, its smallest non-zero value is at least 1e-30 (no denormals: the bound is
relative), at most 60 % of it is exact zeros, and the fp32 twin lies inside the bound.
"""
import collections
import functools

import numpy as np

Spec = collections.namedtuple("Spec", "fam q s rows nc tset bad b L nuc add n_mass free wide")

EM_RUN = 1024                       # positions per wave run of hmm_gene_emissions (csrc/hmm_emitter.inc)
WRAP_POSITIONS = 1024 * 8 * 1024    # grid cap x waves x run: the run loop's stride first executes above this
VARIANTS = {                        # wrong variant -> the family that must tell it from the reference
    "nmass_left": "b",              # n_mass applied on the left side
    "pad0": "b",                    # border padding 0 instead of 1/4
    "swap_right": "a",              # the two minor nucleotides of the right index swapped
    "shift": "b",                   # the window shifted by one position
    "half_n": "c",                  # N counted when the flag is 0.5
    "ge_nc_free": "a",              # state_codon >= nc read as free
    "row_unclamped": "a",           # state_row not clamped (wrapped into the table instead)
    "cross": "b",                   # sequence borders ignored: a 3-mer reads across two sequences
}


def spec_id(spec):
    return "%s-q%d-s%d-r%d-nc%d-%s%d%s-b%d-L%d-%s-add%g-nm%d-f%g" % (
        spec.fam, spec.q, spec.s, spec.rows, spec.nc, "t", spec.tset, ("-bad%d" % spec.bad) if spec.bad else "",
        spec.b, spec.L, spec.nuc, spec.add, spec.n_mass, spec.free) + ("-wide" if spec.wide else "")


def instantiation(q, s, wide):
    """The kernel a call runs: the dispatch of hmm_gene_emissions (csrc/hmm_emitter.inc) restated."""
    if wide:
        return "wide"
    if q <= 16 and 11 <= s <= 16:
        return "<1,1,FAST>"
    if q <= 16 and s <= 16:
        return "<1,1,false>"
    return "<4,2,false>"


def serves(spec, wide):
    """The limits of the two entry points."""
    return (spec.q <= 256 and spec.rows <= 256) if wide else (spec.q <= 64 and spec.rows <= 32)


def bound(s):
    return (s + 140) * 2.0 ** -24


# ---------------------------------------------------------------------------------------------------- inputs

def _softmax(z):
    e = np.exp(z - z.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def _frozen(**arrays):
    for a in arrays.values():
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def tables(q, s, rows, nc, tset, bad=0):
    """B (rows, s) fp32, state_row (q) int32, codon (2, nc, 64) fp32, state_codon (q) int32; read-only."""
    rng = np.random.default_rng([77, q, s, rows, nc, tset])
    B = _softmax(rng.standard_normal((rows, s))).astype(np.float32)
    row = rng.integers(0, rows, q).astype(np.int32)
    codon = (rng.random((2, nc, 64)) * (rng.random((2, nc, 64)) < 0.5)).astype(np.float32)
    free = rng.random(q) < 0.4
    cod = np.where(free, -1, rng.integers(0, max(nc, 1), q)).astype(np.int32)      # (nc = 0: entries 0 >= nc, free too)
    at = (q // 3, q - 1)
    if 1 <= bad <= 3:
        out = (-7, rows, 1 << 20)
        row[at[0]], row[at[1]] = out[bad - 1], out[bad % 3]
    elif bad == 4:
        cod[at[0]], cod[at[1]] = -5, nc + 3
    return _frozen(B=B, row=row, codon=codon, cod=cod)


@functools.lru_cache(maxsize=None)
def inputs(b, L, s, nuc):
    """x (b, L, s + 5) fp32, read-only."""
    rng = np.random.default_rng([99, b, L, s, ("hot", "soft", "place", "placeN").index(nuc)])
    cls = _softmax(2 * rng.standard_normal((b, L, s)))
    idx = rng.integers(0, 4 if nuc == "place" else 5, (b, L))
    nu = np.eye(5)[idx]
    if nuc == "soft":
        kind = rng.random((b, L))
        softrows = _softmax(rng.standard_normal((b, L, 5)))
        nu = np.where((kind < 0.15)[..., None], softrows, nu)                       # genuinely soft rows
        nu[..., 4] = np.where((kind >= 0.15) & (kind < 0.2), 0.5, nu[..., 4])      # N flag != 1
        nu[..., 4] = np.where((kind >= 0.2) & (kind < 0.25), 1.0, nu[..., 4])      # N == 1 next to a base
    elif nuc in ("place", "placeN"):
        softrows = _softmax(rng.standard_normal((b, 5)))
        for i in range(b):
            t = 12 + i
            if t >= L:
                break
            kind = i % 5
            if kind == 0:
                nu[i, t] = softrows[i]
            elif kind == 1:
                nu[i, t, 4] = 0.5
            elif kind == 2:
                nu[i, t] = np.eye(5)[i % 4]
                nu[i, t, 4] = 1.0
            elif kind == 3:
                nu[i, t] = 0.0
            else:
                nu[i, t] = (0.5, 0.5, 0.0, 0.0, 0.0)
    x = np.concatenate([cls, nu], -1).astype(np.float32)
    x.setflags(write=False)
    return x


def build(spec):
    """dict(x, B, row, codon, cod): what the call takes, as read-only numpy arrays."""
    return dict(tables(spec.q, spec.s, spec.rows, spec.nc, spec.tset, spec.bad), x=inputs(spec.b, spec.L, spec.s, spec.nuc))


# ---------------------------------------------------------------------------------------------------- the reference

def reference_arrays(x, B, row, codon, cod, free_value, add, n_mass):
    """The definition in fp64: x (b, L, s + 5), B (rows, s), row (q), codon (2, nc, 64), cod (q) -> E (b, L, q)."""
    x, B, codon = np.asarray(x, np.float64), np.asarray(B, np.float64), np.asarray(codon, np.float64)
    row, cod = np.asarray(row, np.int64), np.asarray(cod, np.int64)
    b, L, w = x.shape
    s, rows, nc, q = w - 5, B.shape[0], codon.shape[1], row.shape[0]
    Bq = B[np.clip(row, 0, rows - 1)]                                   # (q, s)
    free = (cod < 0) | (nc == 0)
    c = np.where(free, 0, np.minimum(cod, nc - 1))
    TL = codon[0][c] if nc else np.zeros((q, 64))                       # (q, 64)
    TR = codon[1][c] if nc else np.zeros((q, 64))
    uniform = np.full(4, 0.25)
    E = np.empty((b, L, q))

    def slot(i, t, mass):
        if t < 0 or t >= L:
            return uniform
        r = x[i, t, s:]
        return r[:4] + (0.25 * mass if r[4] == 1.0 else 0.0)

    for i in range(b):
        for t in range(L):
            emit = Bq @ x[i, t, :s]
            # [n(t+1), n(t+2), n(t)] and [n(t-1), n(t-2), n(t)]: index 16 a + 4 b + c
            left = (slot(i, t + 1, 1.0)[:, None, None] * slot(i, t + 2, 1.0)[None, :, None]
                    * slot(i, t, 1.0)[None, None, :]).reshape(64)
            right = (slot(i, t - 1, n_mass)[:, None, None] * slot(i, t - 2, n_mass)[None, :, None]
                     * slot(i, t, n_mass)[None, None, :]).reshape(64)
            factor = np.where(free, free_value, (TL @ left) * (TR @ right))
            E[i, t] = emit * (factor + add)
    return E


@functools.lru_cache(maxsize=None)
def reference(spec):
    c = build(spec)
    E = reference_arrays(c["x"], c["B"], c["row"], c["codon"], c["cod"], spec.free, spec.add, spec.n_mass)
    E.setflags(write=False)
    return E


def restatement(spec, fp32=False, variant=None):
    """tests/test_emitter_wide_gpu.restatement with the table rules of the header, in fp64 or fp32 torch ops on the
    CPU; variant: one of VARIANTS, a deliberately wrong reading."""
    import torch
    from hmm_layer_amd import kmer
    assert variant is None or variant in VARIANTS
    dtype = torch.float32 if fp32 else torch.float64
    c = build(spec)
    x, B, codon = (torch.from_numpy(np.array(c[k])).to(dtype) for k in ("x", "B", "codon"))
    row, cod = torch.from_numpy(np.array(c["row"])).long(), torch.from_numpy(np.array(c["cod"])).long()
    b, L, s, rows, nc = spec.b, spec.L, spec.s, spec.rows, spec.nc
    row = row % rows if variant == "row_unclamped" else row.clamp(0, rows - 1)
    free = cod < 0
    if variant == "ge_nc_free":
        free = free | (cod >= nc)
    emit = x[..., :s] @ B[row].T
    nuc = x[..., s:]
    if variant == "half_n":
        nuc = nuc.clone()
        nuc[..., 4] = torch.where(nuc[..., 4] == 0.5, torch.ones_like(nuc[..., 4]), nuc[..., 4])
    if variant == "pad0":
        z = torch.zeros((b, 2, 5), dtype=dtype)
        nuc = torch.cat([z, nuc, z], 1)
    elif variant == "cross":
        nuc = nuc.reshape(1, b * L, 5)
    masses = (spec.n_mass, 1) if variant == "nmass_left" else (1, spec.n_mass)
    sides = []
    for left, mass in zip((True, False), masses):
        km = kmer.make_k_mers(nuc, 3, left, n_mass=mass)
        km = km.reshape(km.shape[0], km.shape[1], 64)
        if variant == "pad0":
            km = km[:, 2:-2]
        elif variant == "cross":
            km = km.reshape(b, L, 64)
        if variant == "shift":
            km = torch.cat([km[:, 1:], km[:, -1:]], 1)
        if variant == "swap_right" and not left:
            km = km.reshape(b, L, 4, 4, 4).transpose(2, 3).reshape(b, L, 64)
        sides.append(km)
    if nc:
        ci = cod.clamp(0, nc - 1)
        factor = (sides[0] @ codon[0][ci].T) * (sides[1] @ codon[1][ci].T)
        factor = torch.where(free, torch.full_like(factor, spec.free), factor)
    else:
        factor = torch.full_like(emit, spec.free)
    return (emit * (factor + spec.add)).numpy()


def compare(got, want, s):
    """(worst |got - want| / ((s + 140) 2^-24 want) over want != 0, entries that are zero on one side only)."""
    got, want = np.asarray(got, np.float64), np.asarray(want)
    zero = want == 0
    ratio = np.abs(got - want)[~zero] / (bound(s) * want[~zero])
    return (float(ratio.max()) if ratio.size else 0.0), int(((got == 0) != zero).sum())


def violations(spec):
    """Why the case cannot carry the comparison (empty: it can)."""
    out = []
    want = reference(spec)
    if not np.isfinite(want).all():
        return ["the reference is not finite"]
    nz = want[want != 0]
    if nz.size == 0 or nz.min() < 1e-30:
        out.append("smallest non-zero reference %.3g < 1e-30" % (nz.min() if nz.size else 0.0))
    if (want == 0).mean() > 0.6:
        out.append("%.0f %% exact zeros" % (100 * (want == 0).mean()))
    worst, zeros = compare(restatement(spec, fp32=True), want, spec.s)
    if worst > 1.0 or zeros:
        out.append("fp32 twin: %.3g of the bound, %d zeros differ" % (worst, zeros))
    return out


# ---------------------------------------------------------------------------------------------------- the cases

SETTINGS = ((0.0, 1), (1e-7, 2))                    # (add, n_mass)
FREE = (1.0 / 4096.0, 0.25)
NARROW_Q = (1, 2, 15, 16, 17, 31, 32, 33, 48, 63, 64)
NARROW_S = (1, 3, 4, 10, 11, 12, 15, 16, 17, 20, 31, 32)
NARROW_ROWS, NARROW_NC = (1, 7, 32), (0, 1, 9, 16)
WIDE_Q = (1, 16, 63, 65, 71, 127, 128, 129, 192, 253, 256)
WIDE_S = (1, 7, 15, 16, 17, 32)
WIDE_ROWS, WIDE_NC = (1, 33, 256), (0, 9, 16)
# the four fixed table sets of (b) and (c): (q, s, rows, nc, wide)
TABLE_SETS = {"q15": (15, 15, 13, 9, False), "q7": (7, 7, 5, 9, False), "q29": (29, 20, 32, 16, False),
              "q71w": (71, 15, 61, 9, True)}
SOFT_L = (1, 2, 3, 5, 16, 17, 18, 19, 20, 33, 34)
RUN_EDGES = ((2, 1023), (2, 1024), (2, 1025), (1, 2050), (9, 1000), (1, 8300))


def _bad(k):
    """Every third case two entries of state_row out of range (the three pairs in turn), every third state_codon."""
    return (1 + (k // 3) % 3) if k % 3 == 0 else 4 if k % 3 == 1 else 0


@functools.lru_cache(maxsize=None)
def table_cases(wide):
    out = []
    for qi, q in enumerate(WIDE_Q if wide else NARROW_Q):
        for si, s in enumerate(WIDE_S if wide else NARROW_S):
            k = len(out)
            if wide:
                rows, nc = WIDE_ROWS[(si + qi) % 3], WIDE_NC[(si + si // 3 + qi) % 3]
            else:
                rows, nc = NARROW_ROWS[(si + qi) % 3], NARROW_NC[(si + si // 4 + qi) % 4]
            add, n_mass = SETTINGS[(si + qi) % 2]
            out.append(Spec("a", q, s, rows, nc, 0, _bad(k), 3, 37, "hot", add, n_mass, FREE[(k // 2) % 2], wide))
    return tuple(out)


def _with_tables(name, k, b, L, nuc, fam):
    q, s, rows, nc, wide = TABLE_SETS[name]
    add, n_mass = SETTINGS[k % 2]
    return Spec(fam, q, s, rows, nc, 1, 0, b, L, nuc, add, n_mass, FREE[(k // 2) % 2], wide)


@functools.lru_cache(maxsize=None)
def position_cases(name, block):
    """block: "L1-40" (every L with b = 5, one-hot + N), "soft" (the mixture at SOFT_L), "edges" (RUN_EDGES)."""
    shapes = {"L1-40": [(5, L, "hot") for L in range(1, 41)], "soft": [(5, L, "soft") for L in SOFT_L],
              "edges": [(b, L, "hot") for b, L in RUN_EDGES]}[block]
    return tuple(_with_tables(name, k, b, L, nuc, "b") for k, (b, L, nuc) in enumerate(shapes))


POSITION_BLOCKS = ("L1-40", "soft", "edges")


@functools.lru_cache(maxsize=None)
def placement_cases(name):
    return tuple(_with_tables(name, k, 24, 64, nuc, "c") for k, nuc in enumerate(("place", "placeN")))


def all_cases(fam):
    if fam == "a":
        return table_cases(False) + table_cases(True)
    if fam == "b":
        return tuple(c for name in TABLE_SETS for block in POSITION_BLOCKS for c in position_cases(name, block))
    if fam == "c":
        return tuple(c for name in TABLE_SETS for c in placement_cases(name))
    return tuple(WRAP.values())                     # (d): the single sequence; the device repeats it


# (d): one sequence of L = 1031 (soft mixture), repeated on the device to b = 8200: 8 454 200 positions
WRAP_L, WRAP_B = 1031, 8200
WRAP = {False: Spec("d", 1, 1, 1, 1, 3, 0, 1, WRAP_L, "soft", 1e-7, 2, 0.25, False),
        True: Spec("d", 65, 1, 33, 9, 3, 0, 1, WRAP_L, "soft", 1e-7, 2, 0.25, True)}


# ---------------------------------------------------------------------------------------------------- position logic

def tiles(spec):
    """(P, tb) of every 16-position tile of the call.  Runs start at multiples of the run length, which is a multiple
    of 16 in both kernels, so the tiles start at the multiples of 16."""
    return [(P, P % spec.L) for P in range(0, spec.b * spec.L, 16)]


def fast_tile(P, tb, L, npos):
    """em_scale_tile's predicate without the soft mask, from the shape alone."""
    return tb >= 2 and tb + 18 <= L and P + 16 <= npos


def sequences_in_tile(P, L, npos):
    last = min(P + 15, npos - 1)
    return last // L - P // L + 1
