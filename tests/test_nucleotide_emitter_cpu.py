"""The trainable nucleotide factor (trainable_nucleotides_at_exons=True) without a device: the torch path against a
hand-written fp64 formula, gradients, the start value, config, and the argument checks of hmm_nucleotide_emissions and
hmm_nucleotide_emissions_grad in their order."""
import ctypes

import pytest
import torch

from hmm_layer_amd import build as hbuild
from hmm_layer_amd import engine
from hmm_layer_amd.gene_pred_hmm_emitter import GenePredHMMEmitter

OK, BAD_SHAPE, Q_UNSUPPORTED, NULL_POINTER, WORKSPACE, BAD_ARGUMENT = 0, -1, -2, -3, -4, -6
CODONS = dict(start_codons=[("ATG", 1.)], stop_codons=[("TAG", .34), ("TAA", .33), ("TGA", .33)],
              intron_begin_pattern=[("NGT", .99), ("NGC", .005), ("NAT", .005)],
              intron_end_pattern=[("AGN", .99), ("ACN", .01)])


# ------------------------------------------------------------------------------------------------ module semantics

def make_nucleotides(b, L, g):
    """One-hot rows with N, soft rows, N flags that are not 1, N next to a base, and all-zero rows (padding)."""
    nuc = torch.nn.functional.one_hot(torch.randint(0, 5, (1, b, L), generator=g), 5).float()
    kind = torch.rand((1, b, L), generator=g)
    softrows = torch.softmax(torch.randn((1, b, L, 5), generator=g), -1)
    nuc = torch.where((kind < 0.2)[..., None], softrows, nuc)
    nuc[..., 4] = torch.where((kind >= 0.2) & (kind < 0.3), torch.full_like(kind, 0.5), nuc[..., 4])
    nuc[..., 4] = torch.where((kind >= 0.3) & (kind < 0.4), torch.ones_like(kind), nuc[..., 4])
    nuc = torch.where(((kind >= 0.4) & (kind < 0.5))[..., None], torch.zeros_like(nuc), nuc)
    nuc[0, 0, 0] = torch.tensor([0., 0., 1., 0., 0.])            # each kind at least once, whatever the draw
    nuc[0, 0, 1] = torch.tensor([0., 0., 0., 0., 1.])
    nuc[0, 0, 2] = torch.tensor([.1, .2, .3, .15, .25])
    nuc[0, 0, 3] = 0.0
    return nuc


def make_pair(g, d=None, **kw):
    """(emitter with the option, its twin without) sharing every other parameter."""
    emb = dict(emit_embeddings=True, embedding_dim=d, temperature=float(d)) if d else {}
    on = GenePredHMMEmitter(**CODONS, trainable_nucleotides_at_exons=True, **emb, **kw)
    off = GenePredHMMEmitter(**CODONS, **emb, **kw)
    for em in (on, off):
        em.build((1, 2, 9, 15))
    with torch.no_grad():
        on.emission_kernel.copy_(torch.randn(on.emission_kernel.shape, generator=g))
        off.emission_kernel.copy_(on.emission_kernel)
        if d:
            on.embedding_emission_kernel.copy_(torch.randn(on.embedding_emission_kernel.shape, generator=g))
            off.embedding_emission_kernel.copy_(on.embedding_emission_kernel)
        on.nuc_emission_kernel.copy_(torch.randn(on.nuc_emission_kernel.shape, generator=g))
    return on, off


def make_x(b, L, d, g):
    parts = [torch.softmax(2 * torch.randn((1, b, L, 15), generator=g), -1)]
    if d:
        parts.append(torch.randn((1, b, L, d), generator=g))
    parts.append(make_nucleotides(b, L, g))
    return torch.cat(parts, -1)


def hand_factor(kernel, nuc, c):
    """The issue's formula in fp64, element by element: (b, L, 5) nucleotides -> (b, L, 1 + 14 c)."""
    ker = kernel.detach().double()[0]                                # (3c, 4)
    P = torch.exp(ker) / torch.exp(ker).sum(-1, keepdim=True)
    nuc = nuc.double()
    b, L = nuc.shape[:2]
    q = 1 + 14 * c
    f = torch.full((b, L, q), 0.25, dtype=torch.float64)
    for j in range(1 + 3 * c, 1 + 6 * c):
        r = j - (1 + 3 * c)
        acc = torch.zeros((b, L), dtype=torch.float64)
        for a in range(4):
            acc = acc + (nuc[..., a] + nuc[..., 4] / 4) * P[r, a]
        f[..., j] = acc
    return f


@pytest.mark.parametrize("copies,shared", [(1, True), (1, False), (2, True), (2, False), (3, True), (3, False)])
@pytest.mark.parametrize("training", [False, True])
@pytest.mark.parametrize("d", [None, 4])
@pytest.mark.parametrize("with_hints", [False, True])
def test_module_matches_hand_written_formula(copies, shared, training, d, with_hints):
    """forward() with the option = forward() of the twin without it (everything else of the emitter, tested
    elsewhere) times the hand-written factor, in fp64: relative 1e-12, zeros exact."""
    g = torch.Generator().manual_seed(31 + 7 * copies + int(shared))
    b, L = 2, 9
    on, off = make_pair(g, d, num_copies=copies, share_intron_parameters=shared)
    x = make_x(b, L, d, g)
    hints = torch.rand((1, b, 2, on.num_states), generator=g).double() if with_hints else None
    on, off = on.double(), off.double()
    on.recurrent_init()
    off.recurrent_init()
    with torch.no_grad():
        got = on(x.double(), end_hints=hints, training=training)
        base = off(x.double(), end_hints=hints, training=training)
    f = hand_factor(on.nuc_emission_kernel, x[0][..., -5:], copies)
    want = base * f[None]
    assert tuple(got.shape) == (1, b, L, 1 + 14 * copies)
    assert float(want.max()) > 0 and bool(((got - want).abs() <= 1e-12 * want.abs()).all())
    assert bool((f[0, 3] == 0.25).sum() == on.num_states - 3 * copies) and float(f[0, 3].min()) == 0.0   # the zero row


@pytest.mark.parametrize("L", [1, 2])
def test_sequences_of_length_one_and_two(L):
    """forward() serves sequences shorter than a 3-mer (uniform padding on both sides), with and without the option."""
    g = torch.Generator().manual_seed(17 + L)
    on, off = make_pair(g, num_copies=2)
    nuc = torch.nn.functional.one_hot(torch.randint(0, 5, (1, 3, L), generator=g), 5).float()
    nuc[0, 1] = torch.softmax(torch.randn((L, 5), generator=g), -1)
    x = torch.cat([torch.softmax(2 * torch.randn((1, 3, L, 15), generator=g), -1), nuc], -1)
    on, off = on.double(), off.double()
    on.recurrent_init()
    off.recurrent_init()
    with torch.no_grad():
        got, base = on(x.double()), off(x.double())
    want = base * hand_factor(on.nuc_emission_kernel, x[0][..., -5:], 2)[None]
    assert tuple(got.shape) == (1, 3, L, 29) and float(want.max()) > 0
    assert bool(((got - want).abs() <= 1e-12 * want.abs()).all())
    hints = torch.rand((1, 3, 2, 29), generator=g).double()          # the first and the last position may be the same one
    with torch.no_grad():
        hinted = on(x.double(), end_hints=hints)
    want = want.clone()
    want[:, :, 0] = want[:, :, 0] * hints[:, :, 0]
    want[:, :, -1] = want[:, :, -1] * hints[:, :, 1]
    assert hinted.shape == want.shape and bool(((hinted - want).abs() <= 1e-12 * want.abs()).all())


def test_nucleotide_kernel_receives_gradient():
    g = torch.Generator().manual_seed(4)
    for d in (None, 4):
        on, _ = make_pair(g, d, num_copies=2)
        x = make_x(3, 7, d, g)
        on.recurrent_init()
        E = on(x, training=True)
        (E * torch.randn(E.shape, generator=g)).sum().backward()
        gk = on.nuc_emission_kernel.grad
        assert gk is not None and tuple(gk.shape) == (1, 6, 4) and bool(torch.isfinite(gk).all())
        assert float(gk.abs().max()) > 0 and float(on.emission_kernel.grad.abs().max()) > 0


def test_start_value_config_and_table():
    init = torch.arange(24, dtype=torch.float32).reshape(1, 6, 4) / 10
    em = GenePredHMMEmitter(**CODONS, num_copies=2, trainable_nucleotides_at_exons=True, nucleotide_kernel_init=init)
    em.build((1, 1, 4, 15))
    assert torch.equal(em.nuc_emission_kernel.detach(), init) and em.nuc_emission_kernel.requires_grad
    assert em.nuc_emission_kernel.data_ptr() != init.data_ptr()
    zero = GenePredHMMEmitter(**CODONS, num_copies=3, trainable_nucleotides_at_exons=True)
    zero.build((1, 1, 4, 15))
    assert tuple(zero.nuc_emission_kernel.shape) == (1, 9, 4) and float(zero.nuc_emission_kernel.detach().abs().max()) == 0.0
    assert bool((zero.get_nucleotide_probs() == 0.25).all())
    off = GenePredHMMEmitter(**CODONS, nucleotide_kernel_init=init[:, :3])
    off.build((1, 1, 4, 15))
    assert off.nuc_emission_kernel is None                               # without the option nothing is created
    cfg = zero.get_config()
    assert cfg["trainable_nucleotides_at_exons"] is True and cfg["nucleotide_kernel_init"] is None
    twin = GenePredHMMEmitter.from_config(cfg)
    assert twin.get_config() == cfg and twin.trainable_nucleotides_at_exons
    for c in (1, 2, 3, 18):
        tab = GenePredHMMEmitter(**CODONS, num_copies=c).nucleotide_table(torch.device("cpu"))
        want = [j - (1 + 3 * c) if 1 + 3 * c <= j < 1 + 6 * c else -1 for j in range(1 + 14 * c)]
        assert tab.dtype == torch.int32 and tab.tolist() == want


@pytest.mark.parametrize("d", [None, 4])
@pytest.mark.parametrize("training", [False, True])
def test_fused_path_steps_aside_on_the_cpu(d, training):
    g = torch.Generator().manual_seed(9)
    on, _ = make_pair(g, d)
    x = make_x(2, 9, d, g)
    assert on.can_fuse(x) is False
    on.recurrent_init()
    want = on(x, training=training)
    got = on.forward_fused_trainable(x, training=training)
    assert got.requires_grad and torch.equal(got.detach(), want.detach())


# ------------------------------------------------------------------------------------------------ the C entry points

@pytest.fixture(scope="module")
def lib():
    hbuild.build()
    return engine.lib()


def fwd(lib, ld=24, b=2, L=3, rows=3, q=15, ptrs=(256,) * 4, multiply=1):
    """hmm_nucleotide_emissions with placeholder device pointers: every call here returns before any HIP call."""
    nuc, P, state_nuc, E = ptrs
    return lib.hmm_nucleotide_emissions(nuc, ld, b, L, P, rows, state_nuc, q, ctypes.c_float(0.25), multiply, E, None)


def grad(lib, ld=24, b=2, L=3, rows=3, q=15, ptrs=(256,) * 7, ws_bytes=0):
    """hmm_nucleotide_emissions_grad likewise; ptrs = (nuc, P, state_nuc, E_in, dE, dE_in, dP), the workspace pointer
    256 unless ptrs has an eighth entry.  ws_bytes = 0 is too small for every legal shape."""
    nuc, P, state_nuc, E_in, dE, dE_in, dP = ptrs[:7]
    ws = ptrs[7] if len(ptrs) > 7 else 256
    return lib.hmm_nucleotide_emissions_grad(nuc, ld, b, L, P, rows, state_nuc, q, ctypes.c_float(0.25), E_in, dE,
                                             dE_in, dP, ws, ws_bytes, None)


def test_symbols_and_abi(lib):
    for name in ("hmm_nucleotide_emissions", "hmm_nucleotide_emissions_grad",
                 "hmm_nucleotide_emissions_grad_workspace_bytes"):
        assert hasattr(lib, name)
    assert lib.hmm_abi_version() == 3 == engine.ABI_VERSION
    assert lib.hmm_nucleotide_emissions_max_states() == 256


def test_forward_error_codes_in_order(lib):
    for kw in (dict(b=0), dict(L=0), dict(rows=0), dict(q=0), dict(ld=4), dict(ld=0), dict(b=-1)):
        assert fwd(lib, **kw) == BAD_SHAPE, kw
    assert fwd(lib, ld=4, q=257, ptrs=(None,) * 4, multiply=2) == BAD_SHAPE               # shape before everything
    assert fwd(lib, ld=5, ptrs=(None,) * 4) == NULL_POINTER                               # ld == 5 is a legal shape
    for kw in (dict(q=257), dict(rows=257)):
        assert fwd(lib, **kw) == Q_UNSUPPORTED, kw
        assert fwd(lib, ptrs=(None,) * 4, multiply=2, **kw) == Q_UNSUPPORTED, kw          # limits before pointers
    for i, name in enumerate(("nuc", "P", "state_nuc", "E")):
        ptrs = [256] * 4
        ptrs[i] = None
        assert fwd(lib, ptrs=tuple(ptrs)) == NULL_POINTER, name
        assert fwd(lib, ptrs=tuple(ptrs), multiply=2) == NULL_POINTER, name               # pointers before multiply
    for m in (2, -1):
        assert fwd(lib, multiply=m) == BAD_ARGUMENT
    assert fwd(lib, rows=256, q=256, multiply=3) == BAD_ARGUMENT                           # the limits themselves pass
    assert fwd(lib, rows=1, q=1, ld=5, b=1, L=1, multiply=3) == BAD_ARGUMENT


def test_grad_error_codes_in_order(lib):
    for kw in (dict(b=0), dict(L=0), dict(rows=0), dict(q=0), dict(ld=4), dict(ld=0), dict(L=-3)):
        assert grad(lib, **kw) == BAD_SHAPE, kw
    assert grad(lib, ld=4, q=257, ptrs=(None,) * 8) == BAD_SHAPE                          # shape before everything
    for kw in (dict(q=257), dict(rows=257)):
        assert grad(lib, **kw) == Q_UNSUPPORTED, kw
        assert grad(lib, ptrs=(None,) * 8, **kw) == Q_UNSUPPORTED, kw                     # limits before pointers
    for i, name in ((0, "nuc"), (1, "P"), (2, "state_nuc"), (4, "dE"), (7, "workspace")):
        ptrs = [256] * 8
        ptrs[i] = None
        assert grad(lib, ptrs=tuple(ptrs)) == NULL_POINTER, name                          # pointers before the workspace size
    assert grad(lib, ptrs=(256, 256, 256, 256, 256, None, None)) == NULL_POINTER          # both outputs NULL
    # E_in and either output alone may be NULL: these reach the workspace check
    for ptrs in ((256, 256, 256, None, 256, 256, 256), (256, 256, 256, 256, 256, None, 256),
                 (256, 256, 256, 256, 256, 256, None)):
        assert grad(lib, ptrs=ptrs) == WORKSPACE, ptrs
    need = lib.hmm_nucleotide_emissions_grad_workspace_bytes(2, 3, 3, 15)
    assert need > 0
    assert grad(lib, ws_bytes=need - 1) == WORKSPACE
    assert grad(lib, ptrs=(256,) * 7 + (128,), ws_bytes=need) == WORKSPACE                # not 256-byte aligned
    assert grad(lib, rows=256, q=256, ld=5) == WORKSPACE                                  # the limits themselves pass
    assert grad(lib, rows=1, q=1, ld=5, b=1, L=1) == WORKSPACE


def test_workspace_query(lib):
    ws = lib.hmm_nucleotide_emissions_grad_workspace_bytes
    for args in ((2, 3, 3, 257), (2, 3, 257, 15), (0, 3, 3, 15), (2, 0, 3, 15), (2, 3, 0, 15), (2, 3, 3, 0),
                 (-1, 3, 3, 15)):
        assert ws(*args) == 0, args
    for b, L, rows, q in ((1, 1, 1, 1), (2, 3, 3, 15), (7, 4099, 54, 253), (1000, 1000, 256, 256)):
        n = ws(b, L, rows, q)
        assert n > 0 and n % 256 == 0, (b, L, rows, q, n)
    for rows, q in ((3, 15), (54, 253), (256, 256)):
        assert ws(1000, 1000, rows, q) == ws(1000, 1000000, rows, q) <= 1024 * rows * 16 + 255   # b L = 1e6 and 1e9
        assert ws(1, 300, rows, q) < ws(1000, 1000, rows, q)


def test_python_entry_points_have_no_cpu_path(lib):
    x = torch.rand(2, 3, 15 + 5)
    P = torch.full((3, 4), 0.25)
    tab = torch.tensor([-1] * 4 + [0, 1, 2] + [-1] * 8, dtype=torch.int32)
    with pytest.raises(engine.EngineError):
        engine.nucleotide_emissions(x, 15, P, tab)
    with pytest.raises(engine.EngineError):
        engine.nucleotide_emissions_grad(x, 15, P, tab, torch.rand(2, 3, 15))
