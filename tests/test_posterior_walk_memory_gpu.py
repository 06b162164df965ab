"""hmm_posterior_walk and hmm_posterior_decode_wide stay inside their buffers: guard-band rows through the harness of
tests/memory_contract.py (checks W1, W2, W3, R1 and P), modelled on tests/test_posterior_decode_mid_memory_gpu.py.
Every row is a normal call; the bands are checked after it.  label is a one-byte output at an odd byte offset, conf an
output at mc.ODD_SHIFT, the workspaces have exactly the queried sizes — for the decode call the walk's workspace and
the parking region —, and the harness fills them differently before every run, so a row also shows that nothing is
read from a workspace before the call has written it.  The "-odd" rows put every fp32 argument at an odd float offset,
what a view of an odd-sized model's tensors hands the kernels.  P compares with the plain call on the same data: for
the walk engine.posterior_walk, for the decode call the C entry point on unpadded tensors (engine.posterior_decode may
compose instead, by hmm_posterior_walk_pays).  The symbols are typed in engine.POSTERIOR_WALK_SIGNATURES, so the
completeness check over that table is here."""
import ctypes

import pytest
import torch

import memory_contract as mc
import memory_contract_table as table
import posterior_walk_cases as cases
from memory_contract_table import F64, U8, Bytes, Ref, Row, STREAM, c_call, dev, t32
from hmm_layer_amd import engine

pytestmark = pytest.mark.gpu
WALK, DECODE = "hmm_posterior_walk", "hmm_posterior_decode_wide"
ODD_BYTES = 1031                         # label: an odd byte offset; conf: mc.ODD_SHIFT, an odd float offset
MODES = dict(prob=engine.POST_PROB, log=engine.POST_LOG, noll=engine.POST_LOG_NO_LL)


def inputs(entry, names, b, L):
    k, q = len(names), int(names[0][1:])
    A, pi = table.models(names)
    E = table.emissions((entry, names), k, b, L, q)
    return (k, b, L, q), t32(A), t32(pi), t32(E)


def walk_build(names, b, L, mode, want_ll=True):
    def build():
        dims, A, pi, E = inputs(WALK, names, b, L)
        args = [mc.Arg("A", "inp", A), mc.Arg("pi", "inp", pi), mc.Arg("E", "inp", E, big=True),
                table.ws_arg("hmm_posterior_walk_workspace_bytes", *dims),
                mc.Arg("out", "out", shape=dims, big=True)]
        if want_ll:
            args.append(mc.Arg("ll", "out", shape=dims[:2], dtype=F64))
        argv = [Ref("A"), Ref("pi"), Ref("E"), *dims, engine.EPS, MODES[mode], Ref("out"), Ref("ll"), Ref("ws"),
                Bytes("ws"), STREAM]

        def wrapper():
            out, ll = engine.posterior_walk(dev(A), dev(pi), dev(E), mode=MODES[mode])
            return dict(out=out, ll=ll) if want_ll else dict(out=out)

        return mc.Spec(WALK, "walk-" + mode, args, wrapper=wrapper), c_call(WALK, argv), lambda rep: None
    return build


def decode_build(names, b, L, classes, want_conf=True):
    def build():
        lib = engine.lib()
        dims, A, pi, E = inputs(DECODE, names, b, L)
        k, q = dims[0], dims[3]
        tab, C = (None, q) if classes is None else classes
        ctab = None if tab is None else (ctypes.c_int * q)(*tab)            # the HOST table: no window
        args = [mc.Arg("A", "inp", A), mc.Arg("pi", "inp", pi), mc.Arg("E", "inp", E, big=True),
                table.ws_arg("hmm_posterior_decode_wide_workspace_bytes", *dims),
                mc.Arg("label", "out", shape=dims[:3], dtype=U8, big=True, shift=ODD_BYTES),
                mc.Arg("ll", "out", shape=(k, b), dtype=F64)]
        if want_conf:
            args.append(mc.Arg("conf", "out", shape=dims[:3], big=True, shift=mc.ODD_SHIFT))
        argv = [Ref("A"), Ref("pi"), Ref("E"), *dims, engine.EPS, ctab, C, Ref("label"), Ref("conf"), Ref("ll"),
                Ref("ws"), Bytes("ws"), STREAM]

        def wrapper():
            Ad, pid, Ed = dev(A), dev(pi), dev(E)
            need = lib.hmm_posterior_decode_wide_workspace_bytes(*dims)
            ws = torch.empty(need, dtype=torch.uint8, device=table.DEV)
            out = dict(label=torch.empty(dims[:3], dtype=torch.uint8, device=table.DEV),
                       ll=torch.empty((k, b), dtype=torch.float64, device=table.DEV))
            if want_conf:
                out["conf"] = torch.empty(dims[:3], dtype=torch.float32, device=table.DEV)
            rc = lib.hmm_posterior_decode_wide(Ad.data_ptr(), pid.data_ptr(), Ed.data_ptr(), *dims, engine.EPS, ctab, C,
                                               out["label"].data_ptr(), out["conf"].data_ptr() if want_conf else None,
                                               out["ll"].data_ptr(), ws.data_ptr(), need, table.stream())
            assert rc == 0, rc
            torch.cuda.synchronize()
            return out

        def route(rep):
            assert int(rep.outputs["label"].max()) < C

        return mc.Spec(DECODE, "decode-wide-C%d%s" % (C, "" if want_conf else "-noconf"), args, wrapper=wrapper), \
            c_call(DECODE, argv), route
    return build


def rows():
    D = engine.OPT_FORCE_DENSE
    g71, g253 = (cases.gene_classes(71), 6), (cases.gene_classes(253), 6)
    r = [Row("walk-g71-b3-L37-%s" % m, WALK, walk_build(("g71",), 3, 37, m)) for m in MODES]
    r += [Row("walk-g71-b3-L37-prob-noll", WALK, walk_build(("g71",), 3, 37, "prob", want_ll=False)),
          Row("walk-g71-b3-L37-log-odd", WALK, table.odd(walk_build(("g71",), 3, 37, "log"))),
          Row("walk-g71-g71-b2-L33-log-dense", WALK, walk_build(("g71", "g71"), 2, 33, "log"), [(D, 1)]),
          Row("walk-d100-b2-L33-noll", WALK, walk_build(("d100",), 2, 33, "noll")),
          Row("walk-d129-b2-L20-prob-odd", WALK, table.odd(walk_build(("d129",), 2, 20, "prob"))),
          Row("walk-g253-b1-L17-log", WALK, walk_build(("g253",), 1, 17, "log")),
          Row("decode-wide-g71-b3-L37", DECODE, decode_build(("g71",), 3, 37, g71)),
          Row("decode-wide-g71-b3-L37-odd", DECODE, table.odd(decode_build(("g71",), 3, 37, g71))),
          Row("decode-wide-g71-b3-L37-noconf", DECODE, decode_build(("g71",), 3, 37, g71, want_conf=False)),
          Row("decode-wide-d100-b2-L33-identity", DECODE, decode_build(("d100",), 2, 33, None)),
          Row("decode-wide-d129-b2-L20-odd", DECODE,
              table.odd(decode_build(("d129",), 2, 20, ([i % 16 for i in range(129)], 16)))),
          Row("decode-wide-g253-b1-L17", DECODE, decode_build(("g253",), 1, 17, g253))]
    return r


@pytest.mark.parametrize("row", rows(), ids=lambda r: r.id)
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
        print("CONTRACT %s %s violations %d" % (row.id, spec.label, len(rep.violations)))
        torch.cuda.synchronize()
        route(rep)
    rep.raise_if_failed()


def test_every_pointer_taking_symbol_of_the_table_has_a_row():
    covered = {e for r in rows() for e in r.entry}
    for name, (restype, argtypes) in engine.POSTERIOR_WALK_SIGNATURES.items():
        takes_pointer = any(a is ctypes.c_void_p for a in argtypes) or restype in (ctypes.c_void_p, ctypes.c_char_p)
        assert (name in covered) == takes_pointer, name
    assert covered == {WALK, DECODE}
