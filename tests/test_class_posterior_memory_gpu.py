"""hmm_class_posterior and hmm_class_posterior_grad stay inside their buffers: guard-band rows through the harness of
tests/memory_contract.py (checks W1, W2, W3, R1 and P), modelled on tests/test_class_posterior_walk_memory_gpu.py.  Every
row is a normal call; every argument lies between guard bands, the inputs must come back unchanged and every output
element written.  The workspaces have exactly the queried sizes — the forward's is hmm_posterior's, the backward's has G'
and the routing sums of log mode behind the state call's layout — and the harness fills them differently before every
run, so a row also shows that nothing is read from a workspace before the call has written it.  The "-odd" rows put
every fp32 argument at an odd float offset.  P compares with engine.class_posterior / engine.class_posterior_grad on the
same data.  The class table is a HOST array and has no window.  The symbols are typed in
engine.CLASS_POSTERIOR_SIGNATURES, so the completeness check over that table is here."""
import ctypes

import pytest
import torch

import memory_contract as mc
import memory_contract_table as table
from memory_contract_table import F64, Bytes, Ref, Row, STREAM, c_call, dev, t32
from hmm_layer_amd import engine

pytestmark = pytest.mark.gpu
FWD, BWD = "hmm_class_posterior", "hmm_class_posterior_grad"


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
                table.ws_arg("hmm_class_posterior_workspace_bytes", *dims)]
        if prob:
            args.append(mc.Arg("prob", "out", shape=dims[:3] + (C,), big=True))
        if log:
            args.append(mc.Arg("logp", "out", shape=dims[:3] + (C,), big=True))
        if want_ll:
            args.append(mc.Arg("ll", "out", shape=dims[:2], dtype=F64))
        argv = [Ref("A"), Ref("pi"), Ref("E"), *dims, engine.EPS, ctab, C, Ref("prob"), Ref("logp"), Ref("ll"),
                Ref("ws"), Bytes("ws"), STREAM]

        def wrapper():
            P, Lg, ll = engine.class_posterior(dev(A), dev(pi), dev(E), tab, C, prob=prob, log=log)
            out = dict(prob=P, logp=Lg, ll=ll)
            return {n: out[n] for n, on in (("prob", prob), ("logp", log), ("ll", want_ll)) if on}

        label = "class-C%d%s%s" % (C, "-prob" if prob else "", "-log" if log else "")
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
        P = engine.class_posterior(dev(A), dev(pi), dev(E), tab, C)[0].cpu()                # the forward's out_prob
        args = [mc.Arg("A", "inp", A), mc.Arg("pi", "inp", pi), mc.Arg("E", "inp", E, big=True),
                mc.Arg("P", "inp", P, big=True), mc.Arg("G", "inp", G, big=True),
                table.ws_arg("hmm_class_posterior_grad_workspace_bytes", *dims, C),
                mc.Arg("dA", "out", shape=(k, q, q)), mc.Arg("dpi", "out", shape=(k, q)),
                mc.Arg("dE", "out", shape=dims, big=True)]
        argv = [Ref("A"), Ref("pi"), Ref("E"), *dims, engine.EPS, int(mode), ctab, C, Ref("P"), Ref("G"), Ref("dA"),
                Ref("dpi"), Ref("dE"), Ref("ws"), Bytes("ws"), STREAM]

        def wrapper():
            return dict(zip(("dA", "dpi", "dE"),
                            engine.class_posterior_grad(dev(A), dev(pi), dev(E), tab, C, dev(G), class_prob=dev(P),
                                                        mode=mode)))

        def diag(arena):                                      # the state call's reader, on this call's workspace
            n = lib.hmm_posterior_grad_serial_count(*dims, arena.ptr("ws"), arena.nbytes("ws"))
            assert 0 <= n <= dims[0] * dims[1], n
            return (int(n),)

        label = "class-grad-C%d-%s" % (C, "log" if mode == engine.POST_LOG else "prob")
        return mc.Spec(BWD, label, args, wrapper=wrapper, diag=diag), c_call(BWD, argv), lambda rep: None
    return build


def rows():
    PROB = engine.POST_PROB
    g15 = ([0] + [1 + (i % 14) // 3 for i in range(14)], 6)
    r16 = ([(5 * i) % 16 for i in range(7)], 16)              # more classes than states
    one = ([0] * 16, 1)
    return [Row("class-g15-b3-L133", FWD, fwd_build(("g15",), 3, 133, g15)),
            Row("class-g15-b3-L133-odd", FWD, table.odd(fwd_build(("g15",), 3, 133, g15))),
            Row("class-g15-b3-L133-prob-only-noll", FWD, fwd_build(("g15",), 3, 133, g15, log=False, want_ll=False)),
            Row("class-g15-b2-L1-log-only", FWD, fwd_build(("g15",), 2, 1, g15, prob=False)),
            Row("class-d7-b5-L50-C16-odd", FWD, table.odd(fwd_build(("d7",), 5, 50, r16))),
            Row("class-d16-s16-b2-L37-one", FWD, fwd_build(("d16", "s16"), 2, 37, one)),
            Row("class-grad-g15-b3-L133", BWD, bwd_build(("g15",), 3, 133, g15)),
            Row("class-grad-g15-b3-L133-odd", BWD, table.odd(bwd_build(("g15",), 3, 133, g15))),
            Row("class-grad-g15-b3-L133-prob", BWD, bwd_build(("g15",), 3, 133, g15, mode=PROB)),
            Row("class-grad-g15-b2-L1", BWD, bwd_build(("g15",), 2, 1, g15)),
            Row("class-grad-d7-b5-L50-C16-prob-odd", BWD, table.odd(bwd_build(("d7",), 5, 50, r16, mode=PROB))),
            Row("class-grad-d16-s16-b2-L37-odd", BWD, table.odd(bwd_build(("d16", "s16"), 2, 37, ([i % 5 for i in range(16)], 5)))),
            Row("class-grad-g15-b3-L133-whole", BWD, bwd_build(("g15",), 3, 133, g15), options=((engine.OPT_PGCHUNK, 0),))]


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
    for name, (restype, argtypes) in engine.CLASS_POSTERIOR_SIGNATURES.items():
        takes_pointer = any(a is ctypes.c_void_p for a in argtypes) or restype in (ctypes.c_void_p, ctypes.c_char_p)
        assert (name in covered) == takes_pointer, name
    assert covered == {FWD, BWD}
