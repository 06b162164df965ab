"""hmm_seqshard_mid_reduce / hmm_seqshard_mid_posterior stay inside their buffers: guard-band rows through the harness
of tests/memory_contract.py, modelled on memory_contract_table.seqshard_build — three slabs, a workspace of exactly the
queried size per slab, the workspace pre-filled before the first call only (the chunk operators and the model verdicts
stay in it by design), the host's all-gather in between.  The padding of the operators and exponents is part of the
contract here (zeros, written on every call), so nothing is masked.  The symbols are typed in
hmm_layer_amd/seqshard_mid.py, not in engine._SIGNATURES, so the completeness check over that module's signature table
is here as well."""
import pytest
import torch

import memory_contract as mc
import memory_contract_table as table
from memory_contract_table import CUTS, I32, F64, Bytes, Ref, Row, STREAM, dev, invoke, t32
from hmm_layer_amd import engine, seqshard_mid

pytestmark = pytest.mark.gpu
ENTRY = ("hmm_seqshard_mid_reduce", "hmm_seqshard_mid_posterior")


def mid_build(name, mode):
    def build():
        lib = seqshard_mid.lib()                             # types the symbols on engine.lib()'s handle
        k, b, q, R = 1, 3, int(name[1:]), len(CUTS) - 1
        QT = lib.hmm_seqshard_mid_tile(q)
        A, pi = table.models((name,))
        E = table.emissions(("seqshard_mid", name), k, b, CUTS[-1], q)
        A, pi = t32(A), t32(pi)
        slabs = [t32(E[:, :, CUTS[r]:CUTS[r + 1]]) for r in range(R)]
        args = [mc.Arg("A", "inp", A), mc.Arg("pi", "inp", pi),
                mc.Arg("all_ops", "out", shape=(k, b, R, QT, QT)),
                mc.Arg("all_exps", "out", shape=(k, b, R, QT), dtype=I32)]
        for r in range(R):
            Ls = CUTS[r + 1] - CUTS[r]
            args += [mc.Arg("E%d" % r, "inp", slabs[r], big=True), mc.Arg("op%d" % r, "out", shape=(k, b, QT, QT)),
                     mc.Arg("ex%d" % r, "out", shape=(k, b, QT), dtype=I32),
                     mc.Arg("out%d" % r, "out", shape=(k, b, Ls, q), big=True),
                     mc.Arg("ll%d" % r, "out", shape=(k, b), dtype=F64), mc.Arg("phi%d" % r, "out", shape=(k, b)),
                     table.ws_arg("hmm_seqshard_mid_workspace_bytes", k, b, Ls, q, R, name="ws%d" % r)]

        def call(arena):
            for r in range(R):
                Ls = CUTS[r + 1] - CUTS[r]
                invoke(arena, "hmm_seqshard_mid_reduce", [Ref("A"), Ref("E%d" % r), k, b, Ls, q, engine.EPS, int(r == 0), R,
                                                          Ref("op%d" % r), Ref("ex%d" % r), Ref("ws%d" % r), Bytes("ws%d" % r),
                                                          STREAM])
                arena.check("hmm_seqshard_mid_reduce of slab %d" % r)
            for r in range(R):
                arena.view("all_ops")[:, :, r].copy_(arena.view("op%d" % r))
                arena.view("all_exps")[:, :, r].copy_(arena.view("ex%d" % r))
            for r in range(R):
                Ls = CUTS[r + 1] - CUTS[r]
                invoke(arena, "hmm_seqshard_mid_posterior", [Ref("A"), Ref("pi"), Ref("E%d" % r), k, b, Ls, q, engine.EPS,
                                                             int(r == 0), Ref("all_ops"), Ref("all_exps"), R, r, mode,
                                                             Ref("out%d" % r), Ref("ll%d" % r), Ref("phi%d" % r),
                                                             Ref("ws%d" % r), Bytes("ws%d" % r), STREAM])
                arena.check("hmm_seqshard_mid_posterior of slab %d" % r)

        def wrapper():
            streams = [torch.cuda.Stream() for _ in range(R)]        # one cached workspace per stream = per slab
            res, red = {}, []
            torch.cuda.synchronize()
            for r in range(R):
                with torch.cuda.stream(streams[r]):
                    red.append(seqshard_mid.reduce(dev(A), dev(slabs[r]), r == 0, R))
            torch.cuda.synchronize()
            all_ops = torch.stack([o for o, _ in red], dim=2).contiguous()
            all_exps = torch.stack([e for _, e in red], dim=2).contiguous()
            torch.cuda.synchronize()
            for r in range(R):
                with torch.cuda.stream(streams[r]):
                    o, ll, phi = seqshard_mid.posterior(dev(A), dev(pi), dev(slabs[r]), all_ops, all_exps, r, mode)
                res.update({"op%d" % r: red[r][0], "ex%d" % r: red[r][1], "out%d" % r: o, "ll%d" % r: ll, "phi%d" % r: phi})
            torch.cuda.synchronize()
            return res

        def route(rep):
            assert 16 < q <= lib.hmm_seqshard_mid_max_states()
            for r in range(R):                                        # the scan serves every sequence; zero padding
                assert float(rep.outputs["phi%d" % r].max()) <= 1e-6
                op, ex = rep.outputs["op%d" % r], rep.outputs["ex%d" % r]
                assert not op[..., q:, :].any() and not op[..., :, q:].any() and not ex[..., q:].any()

        spec = mc.Spec(ENTRY, "R3-mode%d" % mode, args, wrapper=wrapper, intermediate=("all_ops", "all_exps"),
                       note="workspace pre-fill before the first call only")
        return spec, call, route
    return build


def rows():
    C, D = engine.OPT_CHUNK, engine.OPT_FORCE_DENSE
    return [Row("seqshard_mid-g29-dense0", ENTRY, mid_build("g29", engine.POST_PROB), [(C, 16), (D, 0)]),
            Row("seqshard_mid-g29-dense1", ENTRY, mid_build("g29", engine.POST_LOG), [(C, 16), (D, 1)]),
            Row("seqshard_mid-d64", ENTRY, mid_build("d64", engine.POST_LOG_NO_LL), [(C, 16)]),
            # alignment pass: every other 4-byte-element argument at an odd float offset; the hops read all_ops as f4
            Row("seqshard_mid-g29-odd", ENTRY, table.odd(mid_build("g29", engine.POST_PROB), keep=("all_ops",)), [(C, 16)])]


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


def test_every_pointer_taking_symbol_of_the_module_has_a_row():
    import ctypes
    covered = {e for r in rows() for e in r.entry}
    for name, (restype, argtypes) in seqshard_mid.SIGNATURES.items():
        takes_pointer = any(a is ctypes.c_void_p for a in argtypes) or restype in (ctypes.c_void_p, ctypes.c_char_p)
        assert (name in covered) == takes_pointer, name
    assert covered == set(ENTRY)
