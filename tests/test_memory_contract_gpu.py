"""Every entry point stays inside its buffers: the guard-band harness (tests/memory_contract.py) over the table of
tests/memory_contract_table.py, entry point x route x shape, on an MI355X.  Each row runs the C entry point on windows
with guard bands and a workspace of exactly the queried size, under every fill, and checks W1 (no write outside),
W2 (every output element written), W3 (no dependence on the workspace's previous contents, diagnostic readers
included), R1 (no byte outside an input reaches a result) and P (bit-identical to the engine.* wrapper), then asserts
that the route the row names was taken.

The alignment rows (ids ending in -odd) place every fp32 / int32 argument at an odd float offset, 256 n + 4 * 1031
bytes — what engine.posterior(A[1:2], pi[1:2], E_all[1:2]) hands the kernels — except the five arguments that need
16 bytes (memory_contract_table.odd); for the two of those that a caller can pass as a view, the wrappers' copy is
tested below.

Measured on an MI355X: the whole file, 807 rows and the tests below them, in 10.4 s (pytest's own figure); the slowest
row, a sequence-sharded Viterbi over three slabs, 0.12 s.
"""
import pytest
import torch

import memory_contract as mc
import memory_contract_table as table

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("row", table.rows(), ids=lambda r: r.id)
def test_row(row):
    with row.applied():
        spec, call, route = row.build()
        assert set(spec.entry) == set(row.entry)
        try:
            rep = mc.run_contract(call, spec, device=table.DEV)
        except RuntimeError as e:                 # a HIP error leaves the device unusable: run nothing after it
            if "HIP error" in str(e) or "hipError" in str(e):
                pytest.exit("HIP error in row %s: %s" % (row.id, e), returncode=3)
            raise
        print("CONTRACT %s %s diag %s violations %d" % (row.id, spec.label, rep.diag, len(rep.violations)))
        torch.cuda.synchronize()
        route(rep)
    rep.raise_if_failed()


def test_the_harness_sees_violations_on_the_device():
    """The checks of tests/test_memory_contract_cpu.py once more where the rows run: a fake entry point made of torch
    ops on the device windows, well-behaved, then with one float written past the workspace (W1), one output element
    left out (W2), a stale workspace float in a result (W3) and a float past an input in a result (R1).  Every access
    stays inside the arena's own buffers."""
    x = torch.rand((5, 7), generator=torch.Generator().manual_seed(3))

    def fake(kind):
        def call(arena):
            ws = arena.view("ws").view(torch.float32)
            stale = ws[40].clone()
            ws[:35] = (3 * arena.view("x")).reshape(-1)
            y = arena.view("y")
            keep = y[4, 6].clone()
            y.copy_(ws[:35].view(5, 7))
            s = arena.slots["ws"]
            if kind == "W1":
                s.buf[s.end:s.end + 4] = 1
            elif kind == "W2":
                y[4, 6] = keep
            elif kind == "W3":
                y[0, 0] += stale * 1e-30
            elif kind == "R1":
                sx = arena.slots["x"]
                y[0, 1] = sx.buf.view(torch.float32)[sx.end // 4]
        return call

    for kind, where in ((None, None), ("W1", "ws"), ("W2", "y"), ("W3", "y"), ("R1", "y")):
        spec = mc.Spec("fake", "device", [mc.Arg("x", "inp", x, big=True), mc.Arg("y", "out", shape=(5, 7), big=True),
                                           mc.Arg("ws", "ws", nbytes=256)], wrapper=lambda: dict(y=3 * x))
        rep = mc.run_contract(fake(kind), spec, device=table.DEV)
        if kind is None:
            assert rep.violations == []
        else:                                     # (a wrong value fails P as well)
            assert {c for c in rep.checks() if c[0] != "P"} == {(kind, where)}, (kind, rep.violations)


def _odd_view(t):
    """The same values in a tensor that starts one float past an allocation's start."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


@pytest.mark.parametrize("name", ["g15", "g29", "s67"])
def test_wrappers_take_views_at_element_alignment(name):
    """engine._dev passes any contiguous view straight through: a view that starts at 4-byte alignment, such as
    E_all[1:2] of a 15-state model, gives what an aligned copy of it gives (include/hmm_engine.h, "Memory contract")."""
    from hmm_layer_amd import engine
    q = int(name[1:])
    A, pi = (table.dev(table.t32(x)) for x in table.models((name,)))
    E = table.dev(table.t32(table.emissions("views", 1, 3, 37, q)))
    G = torch.randn_like(E)
    calls = [lambda A, pi, E, G: engine.posterior(A, pi, E), lambda A, pi, E, G: engine.forward(A, pi, E),
             lambda A, pi, E, G: (engine.backward(A, E),)]
    if q <= 64:
        calls += [lambda A, pi, E, G: engine.loglik_grad(A, pi, E), lambda A, pi, E, G: engine.posterior_grad(A, pi, E, G)]
    else:
        calls += [lambda A, pi, E, G: engine.loglik_grad_large(A, pi, E),
                  lambda A, pi, E, G: engine.posterior_grad_large(A, pi, E, G)]
    for i, fn in enumerate(calls):
        want = fn(A, pi, E, G)
        got = fn(_odd_view(A), _odd_view(pi), _odd_view(E), _odd_view(G))
        torch.cuda.synchronize()
        for x, y in zip(want, got):
            assert torch.equal(x, y), (name, i)
    logs = [A.log(), pi.log(), E.log()]
    for x, y in zip(engine.viterbi(*logs), engine.viterbi(*[_odd_view(t) for t in logs])):
        assert torch.equal(x, y), name


def test_gene_emitter_wrappers_take_views_at_element_alignment():
    from hmm_layer_amd import engine
    B, row, codon, cod, s = table.emitter_tables("default")
    x, g = table.class_and_nucleotides("views", 4, 37, s, True)
    dE = torch.randn((4, 37, row.numel()), generator=g)
    args = [table.dev(t) for t in (x, B, row, codon, cod)]
    odd = [_odd_view(t) for t in args]
    assert torch.equal(engine.gene_emissions(*args), engine.gene_emissions(*odd))
    for x_, y_ in zip(engine.gene_emissions_grad(*args, table.dev(dE)), engine.gene_emissions_grad(*odd, _odd_view(table.dev(dE)))):
        assert torch.equal(x_, y_)


def test_seqshard_wrappers_copy_gathered_operators_that_are_not_16_byte_aligned():
    """all_ops of hmm_seqshard_posterior and all_vops of hmm_seqshard_viterbi_apply are read as aligned 16-byte pieces:
    the wrappers copy a view that starts elsewhere, and return what they return for an aligned tensor."""
    from hmm_layer_amd import engine
    k, b, L, q, R = 1, 3, 40, 15, 1
    A, pi = (table.dev(table.t32(x)) for x in table.models(("g15",)))
    E = table.dev(table.t32(table.emissions("gathered", k, b, L, q)))
    op, ex = engine.seqshard_reduce(A, E, True, R)
    all_ops, all_exps = op.unsqueeze(2).contiguous(), ex.unsqueeze(2).contiguous()
    want = engine.seqshard_posterior(A, pi, E, all_ops, all_exps, 0)
    got = engine.seqshard_posterior(A, pi, E, _odd_view(all_ops), _odd_view(all_exps), 0)
    for x, y in zip(want, got):
        assert torch.equal(x, y)
    whole, _ = engine.posterior(A, pi, E)
    assert float((want[0] - whole).abs().max()) <= 2e-5            # (one slab: the call is the unsharded posterior)
    logs = [A.log(), pi.log(), E.log()]
    vop, vbase = engine.seqshard_viterbi_reduce(*logs, True, R)
    all_vops, all_vbases = vop.unsqueeze(2).contiguous(), vbase.unsqueeze(2).contiguous()
    want = engine.seqshard_viterbi_apply(*logs, all_vops, all_vbases, 0)
    got = engine.seqshard_viterbi_apply(*logs, _odd_view(all_vops), all_vbases, 0)
    for x, y in zip(want, got):
        assert torch.equal(x, y)
