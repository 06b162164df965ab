"""hmm_posterior_decode stays inside its buffers: guard-band rows through the harness of tests/memory_contract.py
(checks W1, W2, W3, R1 and P), modelled on memory_contract_table.rec_build.  label is a one-byte output (the harness
fills it with BYTE_OUT_FILLS), conf and loglik are outputs, the workspace has exactly hmm_workspace_bytes(
HMM_OP_POSTERIOR, ...) bytes.  A chain's first label sits at sequence * L + chunk * T bytes, so the windows of label and
conf start at an odd element offset here, on top of whatever the shape gives.  The symbols are typed in
engine.DECODE_SIGNATURES, not in engine._SIGNATURES, so the completeness check over that table is here as well."""
import ctypes

import pytest
import torch

import memory_contract as mc
import memory_contract_table as table
import posterior_decode_ref as ref
from memory_contract_table import F64, U8, Bytes, Ref, Row, STREAM, c_call, dev, t32
from hmm_layer_amd import engine

pytestmark = pytest.mark.gpu
ENTRY = "hmm_posterior_decode"
ODD_BYTES = 1031                         # label: an odd byte offset; conf: mc.ODD_SHIFT, an odd float offset


def decode_build(names, b, L, classes, want_conf=True, stretch=False, expect=None):
    def build():
        lib = engine.lib()
        k, q = len(names), int(names[0][1:])
        A, pi = table.models(names)
        E = table.emissions((ENTRY, names), k, b, L, q, stretch)
        dims = (k, b, L, q)
        A, pi, E = t32(A), t32(pi), t32(E)
        tab, C = (None, q) if classes is None else classes
        ctab = None if tab is None else (ctypes.c_int * q)(*tab)            # the HOST table: no window
        args = [mc.Arg("A", "inp", A), mc.Arg("pi", "inp", pi), mc.Arg("E", "inp", E, big=True),
                table.ws_arg("hmm_workspace_bytes", engine.OP_POSTERIOR, *dims),
                mc.Arg("label", "out", shape=dims[:3], dtype=U8, big=True, shift=ODD_BYTES),
                mc.Arg("ll", "out", shape=(k, b), dtype=F64)]
        if want_conf:
            args.append(mc.Arg("conf", "out", shape=dims[:3], big=True, shift=mc.ODD_SHIFT))
        argv = [Ref("A"), Ref("pi"), Ref("E"), *dims, engine.EPS, ctab, C, Ref("label"), Ref("conf"), Ref("ll"),
                Ref("ws"), Bytes("ws"), STREAM]

        def wrapper():
            label, conf, ll = engine.posterior_decode(dev(A), dev(pi), dev(E), tab, C, want_conf=want_conf)
            out = dict(label=label, ll=ll)
            if want_conf:
                out["conf"] = conf
            return out

        def diag(arena):
            n = lib.hmm_exact_count(engine.OP_POSTERIOR, *dims, arena.ptr("ws"), arena.nbytes("ws"))
            d = (ctypes.c_longlong * 5)()
            rc = lib.hmm_exact_detail_op(engine.OP_POSTERIOR, *dims, arena.ptr("ws"), arena.nbytes("ws"), d)
            assert n >= 0 and rc == 0, (n, rc)
            return (int(n),) + tuple(int(x) for x in d)

        def route(rep):
            n = rep.diag[0]
            assert (n == 0) if expect == "none" else (0 < n < k * b) if expect == "some" else n == k * b, (n, expect)
            assert int(rep.outputs["label"].max()) < C

        return mc.Spec(ENTRY, "decode-C%d%s" % (C, "" if want_conf else "-noconf"), args, wrapper=wrapper, diag=diag), \
            c_call(ENTRY, argv), route
    return build


def rows():
    C, X = engine.OPT_CHUNK, engine.OPT_EXACT
    gene = (ref.GENE_CLASSES, 5)
    return [Row("decode-g15-b3-L17", ENTRY, decode_build(("g15",), 3, 17, gene, expect="none"), [(C, 16)]),
            Row("decode-d7x2-b5-L333", ENTRY, decode_build(("d7", "d7"), 5, 333, ([0, 1, 1, 2, 2, 2, 0], 3), expect="none"),
                [(C, 16)]),
            Row("decode-d16-b17-L130", ENTRY, decode_build(("d16",), 17, 130, None, expect="none"), [(C, 48)]),
            Row("decode-g15-b3-L17-noconf", ENTRY, decode_build(("g15",), 3, 17, gene, want_conf=False, expect="none"),
                [(C, 16)]),
            # the serial kernels' decode forms: a window around a zero stretch, and every sequence whole
            Row("decode-g15-b3-L100-zeros", ENTRY, decode_build(("g15",), 3, 100, gene, stretch=True, expect="some"),
                [(C, 16), (X, engine.EXACT_AUTO)]),
            Row("decode-g15-b3-L17-always", ENTRY, decode_build(("g15",), 3, 17, gene, expect="all"),
                [(C, 16), (X, engine.EXACT_ALWAYS)])]


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
    for name, (restype, argtypes) in engine.DECODE_SIGNATURES.items():
        takes_pointer = any(a is ctypes.c_void_p for a in argtypes) or restype in (ctypes.c_void_p, ctypes.c_char_p)
        assert (name in covered) == takes_pointer, name
    assert covered == {ENTRY}
