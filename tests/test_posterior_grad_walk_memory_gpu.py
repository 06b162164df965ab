"""hmm_posterior_grad_walk stays inside its buffers: guard-band rows through the harness of tests/memory_contract.py
(checks W1, W2, W3, R1 and P), modelled on tests/test_loglik_grad_walk_memory_gpu.py.  Every row is a normal call in
one of the two modes; every argument lies between guard bands, the inputs must come back unchanged and every output
element written.  The workspace has exactly the queried size and the harness fills it differently before every run, so
a row also shows that nothing is read from the workspace before the call has written it.  The "-odd" rows put every
fp32 argument at an odd float offset.  P compares with engine.posterior_grad_walk on the same data.  The symbols are
typed in engine.POSTERIOR_GRAD_WALK_SIGNATURES, so the completeness check over that table is here
(hmm_posterior_grad_walk_refused takes the workspace of a finished call: each row reads it as its diagnostic)."""
import ctypes

import pytest
import torch

import memory_contract as mc
import memory_contract_table as table
from memory_contract_table import Bytes, Ref, Row, STREAM, c_call, dev, t32
from hmm_layer_amd import engine

pytestmark = pytest.mark.gpu
WALK, REFUSED = "hmm_posterior_grad_walk", "hmm_posterior_grad_walk_refused"


def walk_build(names, b, L, mode=engine.POST_LOG):
    def build():
        lib = engine.lib()
        k, q = len(names), int(names[0][1:])
        dims = (k, b, L, q)
        A, pi = table.models(names)
        A, pi, E = t32(A), t32(pi), t32(table.emissions((WALK, names), k, b, L, q))
        G = t32(table.rng_of("G", names, b, L).standard_normal(dims))
        args = [mc.Arg("A", "inp", A), mc.Arg("pi", "inp", pi), mc.Arg("E", "inp", E, big=True),
                mc.Arg("G", "inp", G, big=True), table.ws_arg("hmm_posterior_grad_walk_workspace_bytes", *dims),
                mc.Arg("dA", "out", shape=(k, q, q)), mc.Arg("dpi", "out", shape=(k, q)),
                mc.Arg("dE", "out", shape=dims, big=True)]
        argv = [Ref("A"), Ref("pi"), Ref("E"), *dims, engine.EPS, int(mode), Ref("G"), Ref("dA"), Ref("dpi"), Ref("dE"),
                Ref("ws"), Bytes("ws"), STREAM]

        def wrapper():
            return dict(zip(("dA", "dpi", "dE"),
                            engine.posterior_grad_walk(dev(A), dev(pi), dev(E), dev(G), mode=mode)))

        def diag(arena):
            n = lib.hmm_posterior_grad_walk_refused(*dims, arena.ptr("ws"), arena.nbytes("ws"))
            assert n >= 0, n
            return (int(n),)

        def route(rep):
            assert rep.diag[0] == 0                                # every model of these rows is served

        label = "pgwalk-%s" % ("log" if mode == engine.POST_LOG else "prob")
        return mc.Spec((WALK, REFUSED), label, args, wrapper=wrapper, diag=diag), c_call(WALK, argv), route
    return build


def rows():
    e = (WALK, REFUSED)
    return [Row("pgwalk-g71-b3-L37", e, walk_build(("g71",), 3, 37)),
            Row("pgwalk-g71-b3-L37-odd", e, table.odd(walk_build(("g71",), 3, 37))),
            Row("pgwalk-g71-b3-L37-prob", e, walk_build(("g71",), 3, 37, mode=engine.POST_PROB)),
            Row("pgwalk-g71-b2-L1", e, walk_build(("g71",), 2, 1)),
            Row("pgwalk-g127-g127-b2-L33", e, walk_build(("g127", "g127"), 2, 33)),
            Row("pgwalk-g127-b65-L9-prob-odd", e, table.odd(walk_build(("g127",), 65, 9, mode=engine.POST_PROB))),
            Row("pgwalk-g253-b1-L17", e, walk_build(("g253",), 1, 17)),
            Row("pgwalk-g253-b2-L8-odd", e, table.odd(walk_build(("g253",), 2, 8)))]


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
    for name, (restype, argtypes) in engine.POSTERIOR_GRAD_WALK_SIGNATURES.items():
        takes_pointer = any(a is ctypes.c_void_p for a in argtypes) or restype in (ctypes.c_void_p, ctypes.c_char_p)
        assert (name in covered) == takes_pointer, name
    assert covered == {WALK, REFUSED}
