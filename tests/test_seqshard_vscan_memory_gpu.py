"""hmm_seqshard_vscan_reduce / _apply / _path stay inside their buffers: guard-band rows through the harness of
tests/memory_contract.py, modelled on memory_contract_table.seqshard_viterbi_build — three slabs, a workspace of exactly
the queried size per slab, the workspace pre-filled before the first call only (the chunk operators, entering scores,
maps and backpointers stay in it by design), the host's two all-gathers in between.  The lanes from q on of the bases
and the maps are left out of the comparisons.  The symbols are typed in hmm_layer_amd/seqshard_vscan.py, not in
engine._SIGNATURES, so the completeness check over that module's signature table is here as well."""
import pytest
import torch

import memory_contract as mc
import memory_contract_table as table
from memory_contract_table import CUTS, I32, I64, U8, F64, Bytes, Ref, Row, STREAM, dev, invoke, lanes_below, t32
from hmm_layer_amd import engine, seqshard_vscan

pytestmark = pytest.mark.gpu
ENTRY = ("hmm_seqshard_vscan_reduce", "hmm_seqshard_vscan_apply", "hmm_seqshard_vscan_path")


def vscan_build(name):
    def build():
        import numpy as np
        lib = seqshard_vscan.lib()                           # types the symbols on engine.lib()'s handle
        k, b, q, R = 1, 3, int(name[1:]), len(CUTS) - 1
        QT = lib.hmm_seqshard_vscan_tile(q)
        logA, logpi = table.log_model((name,))
        logE = np.log(table.emissions(("seqshard_vscan", name), k, b, CUTS[-1], q)).astype(np.float32)
        logA, logpi = t32(logA), t32(logpi)
        slabs = [t32(logE[:, :, CUTS[r]:CUTS[r + 1]]) for r in range(R)]
        args = [mc.Arg("A", "inp", logA), mc.Arg("pi", "inp", logpi),
                mc.Arg("all_vops", "out", shape=(k, b, R, QT, QT), dtype=I32),
                mc.Arg("all_vbases", "out", shape=(k, b, R, QT), dtype=I64, mask=lanes_below(q, k, b, R, QT), loose=True),
                mc.Arg("all_origins", "out", shape=(k, b, R, QT), dtype=U8, mask=lanes_below(q, k, b, R, QT), loose=True)]
        for r in range(R):
            Ls = CUTS[r + 1] - CUTS[r]
            args += [mc.Arg("E%d" % r, "inp", slabs[r], big=True), mc.Arg("vop%d" % r, "out", shape=(k, b, QT, QT), dtype=I32),
                     mc.Arg("vbase%d" % r, "out", shape=(k, b, QT), dtype=I64, mask=lanes_below(q, k, b, QT), loose=True),
                     mc.Arg("origin%d" % r, "out", shape=(k, b, QT), dtype=U8, mask=lanes_below(q, k, b, QT), loose=True),
                     mc.Arg("final%d" % r, "out", shape=(k, b), dtype=I32), mc.Arg("score%d" % r, "out", shape=(k, b), dtype=F64),
                     mc.Arg("path%d" % r, "out", shape=(k, b, Ls), dtype=I32, big=True),
                     table.ws_arg("hmm_seqshard_vscan_workspace_bytes", k, b, Ls, q, R, name="ws%d" % r)]

        def call(arena):
            Ls = [CUTS[r + 1] - CUTS[r] for r in range(R)]
            for r in range(R):
                invoke(arena, "hmm_seqshard_vscan_reduce", [Ref("A"), Ref("pi"), Ref("E%d" % r), k, b, Ls[r], q, int(r == 0), R,
                                                            Ref("vop%d" % r), Ref("vbase%d" % r), Ref("ws%d" % r),
                                                            Bytes("ws%d" % r), STREAM])
                arena.check("hmm_seqshard_vscan_reduce of slab %d" % r)
            for r in range(R):
                arena.view("all_vops")[:, :, r].copy_(arena.view("vop%d" % r))
                arena.view("all_vbases")[:, :, r].copy_(arena.view("vbase%d" % r))
            for r in range(R):
                invoke(arena, "hmm_seqshard_vscan_apply", [Ref("A"), Ref("pi"), Ref("E%d" % r), k, b, Ls[r], q, int(r == 0),
                                                           Ref("all_vops"), Ref("all_vbases"), R, r, Ref("origin%d" % r),
                                                           Ref("final%d" % r), Ref("score%d" % r), Ref("ws%d" % r),
                                                           Bytes("ws%d" % r), STREAM])
                arena.check("hmm_seqshard_vscan_apply of slab %d" % r)
            for r in range(R):
                arena.view("all_origins")[:, :, r].copy_(arena.view("origin%d" % r))
            for r in range(R):
                invoke(arena, "hmm_seqshard_vscan_path", [k, b, Ls[r], q, Ref("all_origins"), Ref("final%d" % r), R, r,
                                                          Ref("path%d" % r), Ref("ws%d" % r), Bytes("ws%d" % r), STREAM])
                arena.check("hmm_seqshard_vscan_path of slab %d" % r)

        def wrapper():
            streams = [torch.cuda.Stream() for _ in range(R)]
            res = {}
            A_, pi_, E_ = dev(logA), dev(logpi), [dev(x) for x in slabs]
            torch.cuda.synchronize()
            red, app = [], []
            for r in range(R):
                with torch.cuda.stream(streams[r]):
                    red.append(seqshard_vscan.reduce(A_, pi_, E_[r], r == 0, R))
            torch.cuda.synchronize()
            all_vops = torch.stack([v for v, _ in red], dim=2).contiguous()
            all_vbases = torch.stack([v for _, v in red], dim=2).contiguous()
            torch.cuda.synchronize()
            for r in range(R):
                with torch.cuda.stream(streams[r]):
                    app.append(seqshard_vscan.apply(A_, pi_, E_[r], all_vops, all_vbases, r))
            torch.cuda.synchronize()
            all_origins = torch.stack([o for o, _, _ in app], dim=2).contiguous()
            torch.cuda.synchronize()
            for r in range(R):
                with torch.cuda.stream(streams[r]):
                    path = seqshard_vscan.path(tuple(E_[r].shape), all_origins, app[r][1], r)
                res.update({"vop%d" % r: red[r][0], "vbase%d" % r: red[r][1], "origin%d" % r: app[r][0],
                            "final%d" % r: app[r][1], "score%d" % r: app[r][2], "path%d" % r: path})
            torch.cuda.synchronize()
            return res

        def route(rep):
            assert 16 < q <= lib.hmm_seqshard_vscan_max_states()
            assert lib.hmm_viterbi_scan_chunk_len(k, b, CUTS[1], q) == 16       # 3, 2 and 4 chunks per slab
            whole, score = engine.viterbi(dev(logA), dev(logpi), dev(t32(logE)))  # the slabs' pieces are the whole path
            assert torch.equal(torch.cat([rep.outputs["path%d" % r] for r in range(R)], dim=2), whole)
            for r in range(R):
                assert torch.equal(rep.outputs["score%d" % r], score)

        spec = mc.Spec(ENTRY, "R3", args, wrapper=wrapper, intermediate=("all_vops", "all_vbases", "all_origins"),
                       note="workspace pre-fill before the first call only")
        return spec, call, route
    return build


def rows():
    C, D = engine.OPT_CHUNK, engine.OPT_FORCE_DENSE
    return [Row("seqshard_vscan-g29-dense0", ENTRY, vscan_build("g29"), [(C, 16), (D, 0)]),
            Row("seqshard_vscan-g29-dense1", ENTRY, vscan_build("g29"), [(C, 16), (D, 1)]),
            Row("seqshard_vscan-g43", ENTRY, vscan_build("g43"), [(C, 16)]),
            # alignment pass: every other 4-byte-element argument at an odd float offset; the hops read all_vops as i4
            Row("seqshard_vscan-g29-odd", ENTRY, table.odd(vscan_build("g29"), keep=("all_vops",)), [(C, 16)])]


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
    for name, (restype, argtypes) in seqshard_vscan.SIGNATURES.items():
        takes_pointer = any(a is ctypes.c_void_p for a in argtypes) or restype in (ctypes.c_void_p, ctypes.c_char_p)
        assert (name in covered) == takes_pointer, name
    assert covered == set(ENTRY)
