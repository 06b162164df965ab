"""hmm_posterior_decode_mid stays inside its buffers: guard-band rows through the harness of tests/memory_contract.py
(checks W1, W2, W3, R1 and P), modelled on tests/test_posterior_decode_memory_gpu.py.  label is a one-byte output at
an odd byte offset, conf an output at mc.ODD_SHIFT, the workspace has exactly
hmm_posterior_decode_mid_workspace_bytes(...) bytes — hmm_posterior's workspace and the walk's parking region —, and
the harness fills it differently before every run, so a row also shows that nothing is read from it before the call
has written it.  The symbols are typed in engine.DECODE_MID_SIGNATURES, so the completeness check over that table is
here."""
import ctypes

import pytest
import torch

import memory_contract as mc
import memory_contract_table as table
import posterior_decode_mid_cases as cases
from memory_contract_table import F64, U8, Bytes, Ref, Row, STREAM, c_call, dev, t32
from hmm_layer_amd import engine

pytestmark = pytest.mark.gpu
ENTRY = "hmm_posterior_decode_mid"
QUERY = "hmm_posterior_decode_mid_workspace_bytes"
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
                table.ws_arg(QUERY, *dims),
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
            assert n >= 0, n
            return (int(n),)

        def route(rep):
            n = rep.diag[0]
            assert (0 < n < k * b) if expect == "some" else n == k * b if expect == "all" else n == 0, (n, expect)
            assert int(rep.outputs["label"].max()) < C

        return mc.Spec(ENTRY, "decode-mid-C%d%s" % (C, "" if want_conf else "-noconf"), args, wrapper=wrapper,
                       diag=diag), c_call(ENTRY, argv), route
    return build


def rows():
    C, X = engine.OPT_CHUNK, engine.OPT_EXACT
    g29, g43 = (cases.gene_classes(29), 6), (cases.gene_classes(43), 6)
    return [Row("decode-mid-g29-b3-L37", ENTRY, decode_build(("g29",), 3, 37, g29, expect="none")),
            Row("decode-mid-d32-b17-L100", ENTRY, decode_build(("d32",), 17, 100, None, expect="none"), [(C, 16)]),
            Row("decode-mid-d64-b2-L300", ENTRY, decode_build(("d64",), 2, 300, ([i % 16 for i in range(64)], 16),
                                                              expect="none"), [(C, 16)]),
            # 43 states, short sequences: by the plan's rule the walk alone (D = 4), which counts no routed sequence
            Row("decode-mid-g43-b3-L37", ENTRY, decode_build(("g43",), 3, 37, g43, expect="none")),
            # scan and walk side by side: the certificate routes the sequence with the zero stretch
            Row("decode-mid-g29-b3-L100-zeros", ENTRY, decode_build(("g29",), 3, 100, g29, stretch=True, expect="some"),
                [(C, 16), (X, engine.EXACT_AUTO)]),
            Row("decode-mid-g29-b3-L37-always", ENTRY, decode_build(("g29",), 3, 37, g29, expect="all"),
                [(X, engine.EXACT_ALWAYS)]),
            Row("decode-mid-g29-b3-L37-noconf", ENTRY, decode_build(("g29",), 3, 37, g29, want_conf=False, expect="none"))]


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
    for name, (restype, argtypes) in engine.DECODE_MID_SIGNATURES.items():
        takes_pointer = any(a is ctypes.c_void_p for a in argtypes) or restype in (ctypes.c_void_p, ctypes.c_char_p)
        assert (name in covered) == takes_pointer, name
    assert covered == {ENTRY}
