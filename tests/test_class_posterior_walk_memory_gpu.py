"""hmm_class_posterior_walk and hmm_class_posterior_grad_walk stay inside their buffers: guard-band rows through the
harness of tests/memory_contract.py (checks W1, W2, W3, R1 and P), modelled on tests/test_posterior_walk_memory_gpu.py
and tests/test_posterior_grad_walk_memory_gpu.py.  Every row is a normal call; every argument lies between guard bands,
the inputs must come back unchanged and every output element written.  The workspaces have exactly the queried sizes —
the forward's with its parking region, the backward's with the quotient tensor of log mode behind the state call's
layout — and the harness fills them differently before every run, so a row also shows that nothing is read from a
workspace before the call has written it.  The "-odd" rows put every fp32 argument at an odd float offset.  P compares
with engine.class_posterior_walk / engine.class_posterior_grad_walk on the same data.  The class table is a HOST array
and has no window.  The symbols are typed in engine.CLASS_POSTERIOR_WALK_SIGNATURES, so the completeness check over that
table is here."""
import ctypes

import pytest
import torch

import memory_contract as mc
import memory_contract_table as table
import posterior_decode_mid_cases as dm
from memory_contract_table import F64, Bytes, Ref, Row, STREAM, c_call, dev, t32
from hmm_layer_amd import engine

pytestmark = pytest.mark.gpu
FWD, BWD = "hmm_class_posterior_walk", "hmm_class_posterior_grad_walk"


def inputs(entry, names, b, L):
    k, q = len(names), int(names[0][1:])
    A, pi = table.models(names)
    return (k, b, L, q), t32(A), t32(pi), t32(table.emissions((entry, names), k, b, L, q))


def fwd_build(names, b, L, classes, prob=True, log=True, want_ll=True):
    def build():
        dims, A, pi, E = inputs(FWD, names, b, L)
        tab, C = classes
        ctab = (ctypes.c_int * dims[3])(*tab)
        args = [mc.Arg("A", "inp", A), mc.Arg("pi", "inp", pi), mc.Arg("E", "inp", E, big=True),
                table.ws_arg("hmm_class_posterior_walk_workspace_bytes", *dims)]
        if prob:
            args.append(mc.Arg("prob", "out", shape=dims[:3] + (C,), big=True))
        if log:
            args.append(mc.Arg("logp", "out", shape=dims[:3] + (C,), big=True))
        if want_ll:
            args.append(mc.Arg("ll", "out", shape=dims[:2], dtype=F64))
        argv = [Ref("A"), Ref("pi"), Ref("E"), *dims, engine.EPS, ctab, C, Ref("prob"), Ref("logp"), Ref("ll"),
                Ref("ws"), Bytes("ws"), STREAM]

        def wrapper():
            P, Lg, ll = engine.class_posterior_walk(dev(A), dev(pi), dev(E), tab, C, prob=prob, log=log)
            out = dict(prob=P, logp=Lg, ll=ll)
            return {n: out[n] for n, on in (("prob", prob), ("logp", log), ("ll", want_ll)) if on}

        label = "class-walk-C%d%s%s" % (C, "-prob" if prob else "", "-log" if log else "")
        return mc.Spec(FWD, label, args, wrapper=wrapper), c_call(FWD, argv), lambda rep: None
    return build


def bwd_build(names, b, L, classes, mode=engine.POST_LOG):
    def build():
        lib = engine.lib()
        dims, A, pi, E = inputs(BWD, names, b, L)
        k, q = dims[0], dims[3]
        tab, C = classes
        ctab = (ctypes.c_int * q)(*tab)
        G = t32(table.rng_of("Gc", names, b, L, C).standard_normal(dims[:3] + (C,)))
        P = engine.class_posterior_walk(dev(A), dev(pi), dev(E), tab, C)[0].cpu()          # the forward's out_prob
        args = [mc.Arg("A", "inp", A), mc.Arg("pi", "inp", pi), mc.Arg("E", "inp", E, big=True),
                mc.Arg("P", "inp", P, big=True), mc.Arg("G", "inp", G, big=True),
                table.ws_arg("hmm_class_posterior_grad_walk_workspace_bytes", *dims, C),
                mc.Arg("dA", "out", shape=(k, q, q)), mc.Arg("dpi", "out", shape=(k, q)),
                mc.Arg("dE", "out", shape=dims, big=True)]
        argv = [Ref("A"), Ref("pi"), Ref("E"), *dims, engine.EPS, int(mode), ctab, C, Ref("P"), Ref("G"), Ref("dA"),
                Ref("dpi"), Ref("dE"), Ref("ws"), Bytes("ws"), STREAM]

        def wrapper():
            return dict(zip(("dA", "dpi", "dE"),
                            engine.class_posterior_grad_walk(dev(A), dev(pi), dev(E), tab, C, dev(G), class_prob=dev(P),
                                                             mode=mode)))

        def diag(arena):                                      # the state call's reader, on this call's workspace
            n = lib.hmm_posterior_grad_walk_refused(*dims, arena.ptr("ws"), arena.nbytes("ws"))
            assert n >= 0, n
            return (int(n),)

        def route(rep):
            assert rep.diag[0] == 0                                # every model of these rows is served

        label = "class-grad-walk-C%d-%s" % (C, "log" if mode == engine.POST_LOG else "prob")
        return mc.Spec(BWD, label, args, wrapper=wrapper, diag=diag), c_call(BWD, argv), route
    return build


def rows():
    PROB = engine.POST_PROB
    g71, g127, g253 = ((dm.gene_classes(q), 6) for q in (71, 127, 253))
    r16 = ([i % 16 for i in range(129)], 16)
    return [Row("class-walk-g71-b3-L37", FWD, fwd_build(("g71",), 3, 37, g71)),
            Row("class-walk-g71-b3-L37-odd", FWD, table.odd(fwd_build(("g71",), 3, 37, g71))),
            Row("class-walk-g71-b3-L37-prob-only-noll", FWD, fwd_build(("g71",), 3, 37, g71, log=False, want_ll=False)),
            Row("class-walk-g71-b2-L1-log-only", FWD, fwd_build(("g71",), 2, 1, g71, prob=False)),
            Row("class-walk-d129-b2-L20-C16-odd", FWD, table.odd(fwd_build(("d129",), 2, 20, r16))),
            Row("class-walk-g253-b1-L17", FWD, fwd_build(("g253",), 1, 17, g253)),
            Row("class-grad-walk-g71-b3-L37", BWD, bwd_build(("g71",), 3, 37, g71)),
            Row("class-grad-walk-g71-b3-L37-odd", BWD, table.odd(bwd_build(("g71",), 3, 37, g71))),
            Row("class-grad-walk-g71-b3-L37-prob", BWD, bwd_build(("g71",), 3, 37, g71, mode=PROB)),
            Row("class-grad-walk-g71-b2-L1", BWD, bwd_build(("g71",), 2, 1, g71)),
            Row("class-grad-walk-g127-g127-b2-L33", BWD, bwd_build(("g127", "g127"), 2, 33, g127)),
            Row("class-grad-walk-g127-b65-L9-prob-odd", BWD, table.odd(bwd_build(("g127",), 65, 9, g127, mode=PROB))),
            Row("class-grad-walk-g253-b2-L8-odd", BWD, table.odd(bwd_build(("g253",), 2, 8, g253)))]


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
    for name, (restype, argtypes) in engine.CLASS_POSTERIOR_WALK_SIGNATURES.items():
        takes_pointer = any(a is ctypes.c_void_p for a in argtypes) or restype in (ctypes.c_void_p, ctypes.c_char_p)
        assert (name in covered) == takes_pointer, name
    assert covered == {FWD, BWD}
