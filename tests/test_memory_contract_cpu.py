"""The guard-band harness (tests/memory_contract.py) must be able to fail: it runs here on CPU tensors against fake
entry points, plain Python functions over the arena's windows, one well-behaved and one per kind of violation, and
each violation must be reported under the right check and argument.  The completeness test holds the GPU table
(tests/memory_contract_table.py) against engine._SIGNATURES: an entry point with a pointer argument is either in the
table or in EXEMPT with a reason."""
import ctypes

import pytest
import torch

import memory_contract as mc
import memory_contract_table as table
from hmm_layer_amd import engine

MARGIN = 4096
WS_BYTES = 512


def spec(wrapper=None, diag=None, masked=False):
    g = torch.Generator().manual_seed(5)
    x = torch.rand((8, 6), generator=g)
    mask = None
    if masked:                                           # columns 0 and 5 do not belong to the argument
        mask = torch.ones((8, 6), dtype=torch.bool)
        mask[:, 0] = mask[:, 5] = False
    args = [mc.Arg("x", "inp", x, mask=mask, big=True), mc.Arg("w", "inp", torch.rand(3, generator=g).double()),
            mc.Arg("y", "out", shape=(8, 6), mask=mask, big=True), mc.Arg("ll", "out", shape=(8,), dtype=torch.float64),
            mc.Arg("n", "out", shape=(8,), dtype=torch.int32), mc.Arg("o", "out", shape=(5,), dtype=torch.uint8),
            mc.Arg("acc", "inout", torch.rand((8,), generator=g)), mc.Arg("ws", "ws", nbytes=WS_BYTES)]
    return mc.Spec("fake", "cpu", args, wrapper=wrapper, diag=diag), x


def good(arena, masked=False):
    x, y = arena.view("x"), arena.view("y")
    scratch = arena.view("ws").view(torch.float32)
    scratch[:48] = (2 * x).reshape(-1)                    # initialised before it is read
    scratch[100] = float(x[1, 1])                         # a counter that the diagnostic reads
    if masked:
        y[:, 1:5] = scratch[:48].view(8, 6)[:, 1:5]
    else:
        y.copy_(scratch[:48].view(8, 6))
    cols = x[:, 1:5] if masked else x
    arena.view("ll").copy_(cols.double().sum(1) + arena.view("w").sum())
    arena.view("n").copy_(torch.arange(8, dtype=torch.int32))
    arena.view("o").zero_()
    arena.view("acc").mul_(3.0)


def floats_of(arena, name):
    s = arena.slots[name]
    return s.buf.view(torch.float32), s.start // 4, s.end // 4


def run(call, **kw):
    sp, _ = spec(**kw)
    return mc.run_contract(call, sp, margin_bytes=MARGIN)


def test_well_behaved_call_passes():
    sp, x = spec(wrapper=lambda: dict(y=2 * x, ll=x.double().sum(1) + sp.args[1].data.sum(),
                                       n=torch.arange(8, dtype=torch.int32), o=torch.zeros(5, dtype=torch.uint8),
                                       acc=sp.args[6].data * 3.0),
                 diag=lambda arena: (float(arena.view("ws").view(torch.float32)[100]),))
    rep = mc.run_contract(good, sp, margin_bytes=MARGIN)
    assert rep.violations == []
    rep.raise_if_failed()
    assert torch.equal(rep.outputs["y"], 2 * x) and rep.diag == (float(x[1, 1]),)


def test_windows_are_placed_as_the_header_says():
    sp, _ = spec()
    arena = mc.Arena("cpu", MARGIN)
    for a in sp.args:
        arena.add(a)
    for name, s in arena.slots.items():
        assert s.start >= MARGIN and len(s.buf) - s.end >= MARGIN
        assert s.ptr % 256 == (8 if s.arg.dtype == torch.float64 else 0), name
    assert arena.nbytes("ws") == WS_BYTES and arena.ptr("absent") is None
    odd = mc.Arena("cpu", MARGIN)
    odd.add(mc.Arg("x", "inp", torch.rand(7), shift=mc.ODD_SHIFT))
    assert odd.ptr("x") % 256 == mc.ODD_SHIFT % 256 and odd.ptr("x") % 8 == 4
    # the window is the memory the pointer names
    odd.slots["x"].prepare(mc.NAN_BITS, None)
    got = (ctypes.c_float * 7).from_address(odd.ptr("x"))
    assert list(got) == odd.view("x").tolist()


@pytest.mark.parametrize("where", ["before", "after"])
def test_write_next_to_an_output_is_W1(where):
    def call(arena):
        good(arena)
        raw, first, end = floats_of(arena, "y")
        raw[first - 1 if where == "before" else end] = 1.0
    rep = run(call)
    assert rep.checks() == [("W1", "y")]
    lo = -4 if where == "before" else 8 * 6 * 4                  # the first byte of that float that changed
    assert lo <= rep.violations[0].offset < lo + 4
    with pytest.raises(mc.ContractViolation, match=r"W1: fake \[cpu\], argument y, .*offset %d" % rep.violations[0].offset):
        rep.raise_if_failed()


def test_write_past_the_workspace_is_W1():
    def call(arena):
        good(arena)
        s = arena.slots["ws"]
        s.buf[s.end] = 1
    rep = run(call)
    assert rep.checks() == [("W1", "ws")] and rep.violations[0].offset == WS_BYTES


def test_write_into_an_input_or_a_hole_is_W1():
    def into_input(arena):
        good(arena)
        arena.view("x")[2, 2] = 0.5
    rep = run(into_input)
    assert ("W1", "x") in rep.checks() and rep.violations[0].offset == (2 * 6 + 2) * 4

    def into_hole(arena):
        good(arena, masked=True)
        arena.view("y")[3, 5] = 0.0
    rep = run(into_hole, masked=True)
    assert rep.checks() == [("W1", "y")] and 0 <= rep.violations[0].offset - (3 * 6 + 5) * 4 < 4
    assert run(lambda arena: good(arena, masked=True), masked=True).violations == []


def test_stray_write_between_the_calls_of_a_sequence_is_W1():
    def call(arena):
        good(arena)
        raw, first, end = floats_of(arena, "ll")
        keep = raw[end].clone()
        raw[end] = 2.0
        arena.check("the first call")
        raw[end] = keep                                   # the second call repairs it: only check() between sees it
    rep = run(call)
    assert rep.checks() == [("W1", "ll")] and "the first call" in rep.violations[0].text


@pytest.mark.parametrize("name,index", [("y", (3, 2)), ("ll", (7,)), ("n", (0,)), ("o", (4,))])
def test_unwritten_output_element_is_W2(name, index):
    def call(arena):
        keep = arena.view(name)[index].clone()
        good(arena)
        arena.view(name)[index] = keep
    rep = run(call)
    assert rep.checks() == [("W2", name)]
    assert "was not written" in rep.violations[0].text


def test_uninitialised_workspace_in_a_result_is_W3():
    def call(arena):
        stale = arena.view("ws").view(torch.float32)[77].clone()
        good(arena)
        arena.view("y")[0, 0] += stale * 1e-30
    rep = run(call)
    assert rep.checks() == [("W3", "y")] and rep.violations[0].offset == 0


def test_uninitialised_counter_in_a_diagnostic_is_W3():
    rep = run(good, diag=lambda arena: (int(arena.view("ws").view(torch.int32)[90]),))
    assert rep.checks() == [("W3", "diagnostics")]


def test_read_past_an_input_is_R1():
    def call(arena):
        good(arena)
        raw, first, end = floats_of(arena, "x")
        arena.view("y")[7, 5] = raw[end]
    rep = run(call)
    assert rep.checks() == [("R1", "y")] and rep.violations[0].offset == (7 * 6 + 5) * 4


def test_read_of_an_unused_column_is_R1():
    def call(arena):
        good(arena, masked=True)
        arena.view("ll")[2] += float(arena.view("x")[2, 0])
    rep = run(call, masked=True)
    assert rep.checks() == [("R1", "ll")]


def test_mismatch_with_the_wrapper_is_P():
    sp, x = spec(wrapper=lambda: dict(y=2 * x + 1e-7, ll=torch.zeros(8, dtype=torch.float64)))
    rep = mc.run_contract(good, sp, margin_bytes=MARGIN)
    assert set(rep.checks()) == {("P", a) for a in ("y", "ll", "n", "o", "acc")}


def test_tolerance_fallback_is_per_spec():
    def call(arena):
        stale = arena.view("ws").view(torch.uint8)[300].clone()
        good(arena)
        arena.view("y")[0, 0] += float(stale) * 1e-9
    sp, _ = spec()
    assert mc.run_contract(call, sp, margin_bytes=MARGIN).checks() == [("W3", "y")]
    sp.tol = (1e-6, 0.0)
    assert mc.run_contract(call, sp, margin_bytes=MARGIN).violations == []


# ---- completeness -------------------------------------------------------------------------------------------------
def pointer_entry_points():
    """Symbols that take or return a pointer."""
    return sorted(n for n, (restype, argtypes) in engine._SIGNATURES.items()
                  if ctypes.c_void_p in argtypes or restype in (ctypes.c_void_p, ctypes.c_char_p))


def test_every_pointer_entry_point_is_in_the_table_or_exempt():
    covered = {e for row in table.rows() for e in row.entry}
    for name in pointer_entry_points():
        assert (name in covered) != (name in table.EXEMPT), \
            "%s takes pointers: give it a row in tests/memory_contract_table.py or an EXEMPT entry with a reason" % name
    assert covered <= set(engine._SIGNATURES) and set(table.EXEMPT) <= set(pointer_entry_points())
    for name, reason in table.EXEMPT.items():
        assert isinstance(reason, str) and len(reason) > 10 and "\n" not in reason, name


def test_row_ids_are_unique():
    ids = [r.id for r in table.rows()]
    assert len(ids) == len(set(ids)) and len(ids) > 100
