"""The rows of the memory-contract test (tests/test_memory_contract_gpu.py): entry point x route x shape.

A Row is built lazily on the device machine: Row.build() -> (Spec, call, route), where call(arena) invokes the C entry
point(s) through engine.lib() with the arena's window addresses (the workspace size passed is exactly what the size
query returned), and route(report) asserts from the diagnostic readers, chunk_len and the *_pays predicates that the
row took the route it names.  Row.options are the (engine.OPT_*, value) pairs under which the whole row runs, the
wrapper call of check P included.  Importing this module needs no device: tests/test_memory_contract_cpu.py holds
rows() and EXEMPT against engine._SIGNATURES.

Shapes are the smallest that are ragged in every way the kernels tile: q % 4 != 0 and q at a block edge, b % 16 != 0,
L % 16 != 0 (a short last chunk), more than one wave, and 34 chunks where a route has a two-level scan.
"""
import contextlib
import ctypes
import functools
import zlib

import numpy as np
import torch

import memory_contract as mc
from hmm_layer_amd import engine

# Entry points with pointer arguments that have no row, and why.
EXEMPT = {
    "hmm_strerror": "returns a pointer to a constant host string; takes no pointer",
    "hmm_profile_create": "returns the host-side handle of the profiler; no device memory",
    "hmm_profile_destroy": "host-side handle of the profiler, no device memory",
    "hmm_profile_read": "host-side handle and host arrays of HMM_KERNEL_COUNT entries, no device memory",
    "hmm_posterior_profiled": "hmm_posterior (posterior_impl) with HIP events around its launches: same kernels, same workspace",
    "hmm_loglik_allreduce": "needs an RCCL communicator; the engine only forwards `partial` to ncclAllReduce",
    "hmm_exact_count": "last-call reader: copies one counter per plan to the host; run as a diagnostic under W3",
    "hmm_exact_detail_op": "last-call reader: copies five counters per plan to the host; run as a diagnostic under W3",
    "hmm_window_table": "last-call reader (test hook): copies one sequence's window records into host arrays",
    "hmm_loglik_grad_serial_count": "last-call reader: one counter to the host; run as a diagnostic under W3",
    "hmm_loglik_grad_scan_serial_count": "last-call reader: one counter to the host; run as a diagnostic under W3",
    "hmm_posterior_grad_serial_count": "last-call reader: one counter to the host; run as a diagnostic under W3",
    "hmm_posterior_grad_scan_serial_count": "last-call reader: one counter to the host; run as a diagnostic under W3",
}

CODONS = dict(start_codons=[("ATG", 1.)], stop_codons=[("TAG", .34), ("TAA", .33), ("TGA", .33)],
              intron_begin_pattern=[("NGT", .99), ("NGC", .005), ("NAT", .005)],
              intron_end_pattern=[("AGN", .99), ("ACN", .01)])
F32, F64, I32, I64, U8 = torch.float32, torch.float64, torch.int32, torch.int64, torch.uint8
OPT_NAMES = {engine.OPT_CHUNK: "chunk", engine.OPT_FORCE_DENSE: "dense", engine.OPT_SCAN2: "scan2",
             engine.OPT_EXACT: "exact", engine.OPT_PGCHUNK: "pgchunk", engine.OPT_VGROUPS: "vgroups",
             engine.OPT_VLARGE: "vlarge", engine.OPT_GLARGE: "glarge"}
DEV = "cuda:0"


class Row:
    def __init__(self, id, entry, build, options=()):
        self.id, self.build, self.options = id, build, tuple(options)
        self.entry = (entry,) if isinstance(entry, str) else tuple(entry)

    @contextlib.contextmanager
    def applied(self):
        with contextlib.ExitStack() as stack:
            for opt, value in self.options:
                stack.enter_context(engine.option(opt, value))
            yield


def opt_id(options):
    return "".join("-%s%d" % (OPT_NAMES[o], v) for o, v in options)


def rng_of(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def t32(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))


def dev(t):
    return t.to(DEV)


class Ref:
    """The address of argument `name`'s window plus `offset` bytes; NULL when the row has no such argument."""

    def __init__(self, name, offset=0):
        self.name, self.offset = name, offset


class Bytes:
    def __init__(self, name):
        self.name = name


STREAM = object()


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def invoke(arena, symbol, argv):
    args = []
    for a in argv:
        if isinstance(a, Ref):
            p = arena.ptr(a.name)
            args.append(None if p is None else p + a.offset)
        elif isinstance(a, Bytes):
            args.append(arena.nbytes(a.name))
        elif a is STREAM:
            args.append(stream())
        else:
            args.append(a)
    rc = getattr(engine.lib(), symbol)(*args)
    assert rc == 0, "%s returned %d (%s)" % (symbol, rc, engine.lib().hmm_strerror(rc).decode())


def c_call(symbol, argv):
    return lambda arena: invoke(arena, symbol, argv)


def ws_arg(symbol, *dims, name="ws"):
    need = getattr(engine.lib(), symbol)(*dims)
    assert need > 0, (symbol, dims)
    return mc.Arg(name, "ws", nbytes=need)


def odd(build, keep=()):
    """Alignment pass: the same row with every 4-byte-element argument (not the workspace) at an odd float offset,
    256 n + 4 * 1031 bytes — what engine.posterior(A[1:2], pi[1:2], E_all[1:2]) hands the kernels for an odd-sized model.
    Decided by reading csrc/, every cast to a vector type traced from the kernel parameter to its launch sites: the
    kernels reach caller memory through scalar element accesses, 4-byte-aligned vector types (f4u, P4 / P3 / P2) and raw
    buffer loads, none of which assumes more than element alignment — with five exceptions, all casts to the naturally
    aligned f4 / i4: E of hmm_gene_emissions and dx of hmm_gene_emissions_grad / _grad_wide (em_flush_flat),
    all_ops of hmm_seqshard_posterior (k_scan reads the caller's operator rows as f4) and all_vops of
    hmm_seqshard_viterbi_apply (vit_hops reads them as i4).  Every other such cast lands in the workspace (ops, exps, vops,
    prefix / suffix / xend / rstart, checkpoints, W, backpointers: 256-byte-aligned regions) or in LDS.  keep: the
    arguments of a row that need 16 bytes; they are not run misaligned."""
    def wrapped():
        spec, call, route = build()
        for a in spec.args:
            if a.kind != "ws" and a.itemsize == 4 and a.name not in keep:
                a.shift = mc.ODD_SHIFT
        spec.route += "-odd"
        return spec, call, route
    return wrapped


# ---- models -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def model(name):
    """-> A (q,q), pi (q) float32 numpy.  g15 / g29 / g43: the gene models of one to three copies; dQ: a dense model;
    sQ: a dense model whose rows keep about a tenth of their entries."""
    import postgrad_mid_cases as pm
    from oracle import params
    q = int(name[1:])
    if name == "g15":
        return params.intended_A15().numpy().astype(np.float32), np.full(15, 1 / 15, dtype=np.float32)
    if name[0] == "g":
        A, pi = pm.gene_model((q - 1) // 14)
        return np.array(A), np.array(pi)
    return pm.rand_model(rng_of("model", name), q, sparse=name[0] == "s")


def models(names):
    A, pi = zip(*(model(n) for n in names))
    return np.stack(A), np.stack(pi)


def emissions(key, k, b, L, q, stretch=False):
    E = (rng_of("E", key, k, b, L, q).random((k, b, L, q)) * 0.9 + 0.05).astype(np.float32)
    if stretch:                                              # six all-zero positions in one sequence: the clamp regime
        E[0, min(1, b - 1), L // 2:L // 2 + 6] = 0.0
    if stretch == "only":                                    # ... in which one state alone emits, one that the model
        A = model(key[1][0])[0]                              # leaves after one step for certain (tests/test_grad_gpu.py)
        E[0, min(1, b - 1), L // 2:L // 2 + 6, int(np.argmax((A > 0).sum(-1) == 1))] = 0.5
    return E


def log_model(names):
    A, pi = models(names)
    with np.errstate(divide="ignore"):
        return np.log(A).astype(np.float32), np.log(pi).astype(np.float32)


# ---- forward / backward / posterior ---------------------------------------------------------------------------------
REC_OPS = ("loglik", "forward", "backward", "post_prob", "post_log", "post_noll")
REC_OP = dict(loglik=engine.OP_LOGLIK, forward=engine.OP_FORWARD, backward=engine.OP_BACKWARD,
              post_prob=engine.OP_POSTERIOR, post_log=engine.OP_POSTERIOR, post_noll=engine.OP_POSTERIOR)
REC_ENTRY = dict(loglik="hmm_forward", forward="hmm_forward", backward="hmm_backward", post_prob="hmm_posterior",
                 post_log="hmm_posterior", post_noll="hmm_posterior")
POST_MODE = dict(post_prob=engine.POST_PROB, post_log=engine.POST_LOG, post_noll=engine.POST_LOG_NO_LL)


def rec_build(op, names, b, L, stretch, expect, no_ll=False):
    """expect: how the row's route shows — dict(chunk=T or None, chunks_min=n, exact='none' | 'some' (0 < n < k b: both kinds of kernels side by side) | 'all' | None).
    no_ll: hmm_posterior without its optional loglik output."""
    def build():
        lib = engine.lib()
        k, q = len(names), int(names[0][1:])
        A, pi = models(names)
        E = emissions((op, names), k, b, L, q, stretch)
        dims = (k, b, L, q)
        A, pi, E = t32(A), t32(pi), t32(E)
        args = [mc.Arg("A", "inp", A), mc.Arg("E", "inp", E, big=True),
                ws_arg("hmm_workspace_bytes", REC_OP[op], *dims)]
        if op != "backward":
            args.append(mc.Arg("pi", "inp", pi))
            if not no_ll:
                args.append(mc.Arg("ll", "out", shape=(k, b), dtype=F64))
        if op != "loglik":
            args.append(mc.Arg("out", "out", shape=dims, big=True))
        tail = [Ref("ws"), Bytes("ws"), STREAM]
        if op in ("loglik", "forward"):
            argv = [Ref("A"), Ref("pi"), Ref("E"), *dims, engine.EPS, Ref("out"), Ref("ll")] + tail
            wrapper = lambda: dict(zip(("out", "ll"), engine.forward(dev(A), dev(pi), dev(E), op == "forward")))
        elif op == "backward":
            argv = [Ref("A"), Ref("E"), *dims, engine.EPS, Ref("out")] + tail
            wrapper = lambda: dict(out=engine.backward(dev(A), dev(E)))
        else:
            argv = [Ref("A"), Ref("pi"), Ref("E"), *dims, engine.EPS, POST_MODE[op], Ref("out"), Ref("ll")] + tail
            wrapper = lambda: dict(zip(("out", "ll"), engine.posterior(dev(A), dev(pi), dev(E), mode=POST_MODE[op])))
        if op == "loglik" or no_ll:
            inner = wrapper
            wrapper = lambda: {n: v for n, v in inner().items() if n == ("ll" if op == "loglik" else "out")}

        def diag(arena):
            if q > 64:
                return ()
            n = lib.hmm_exact_count(REC_OP[op], *dims, arena.ptr("ws"), arena.nbytes("ws"))
            assert n >= 0, n
            if q > 16:
                return (int(n),)
            d = (ctypes.c_longlong * 5)()
            rc = lib.hmm_exact_detail_op(REC_OP[op], *dims, arena.ptr("ws"), arena.nbytes("ws"), d)
            assert rc == 0, rc
            return (int(n),) + tuple(int(x) for x in d)

        def route(rep):
            if q <= 16:
                T = lib.hmm_chunk_len(*dims)
                assert T > 0 and (expect.get("chunk") is None or T == expect["chunk"]), T
                assert (L + T - 1) // T >= expect.get("chunks_min", 1), (L, T)
            elif q <= 64:
                assert lib.hmm_chunk_len(*dims) == 0
                # hmm_scan_rows.inc: 33..64 states take the chunked scan for few long sequences only (sparse models
                # up to 56 of them, L >= SCAN64_MIN_LEN = 256); otherwise one wave walks one sequence (hmm_midq.inc)
                assert q <= 32 or (k * b <= 56 and L >= 256) == bool(expect.get("scan64"))
            else:
                assert lib.hmm_largeq_tile_cols(b, q) in (64, 80, 96)
                return
            n = rep.diag[0]
            want = expect.get("exact")
            assert want is None or (n == 0 if want == "none" else n == k * b if want == "all" else 0 < n < k * b), (n, want)

        return mc.Spec(REC_ENTRY[op], op, args, wrapper=wrapper, diag=diag), c_call(REC_ENTRY[op], argv), route
    return build


def recursion_rows():
    out = []
    C, D, S2, X = engine.OPT_CHUNK, engine.OPT_FORCE_DENSE, engine.OPT_SCAN2, engine.OPT_EXACT

    def add(names, b, L, options, expect, stretch=False, ops=REC_OPS, tag="", wrap=lambda build: build, no_ll=False):
        for op in ops:
            out.append(Row("rec-%s-%s-b%d-L%d%s%s" % (op, "+".join(names), b, L, opt_id(options), tag), REC_ENTRY[op],
                           wrap(rec_build(op, names, b, L, stretch, expect, no_ll)), options))

    # up to 16 states: the 16-state scan, compiled (g15) and generic, one- and two-level chunk scans
    for names, dense in ((("g15",), (0, 1)), (("d7",), (0,)), (("d16",), (0,))):
        pair = names + ("d" + names[0][1:],)
        for fd in dense:
            add(names, 3, 37, [(D, fd)], dict(exact="none"))
            add(pair, 17, 100, [(C, 16), (D, fd)], dict(chunk=16, chunks_min=7, exact="none"))
            for two in (1, 0):
                add(names, 2, 530, [(C, 16), (S2, two), (D, fd)], dict(chunk=16, chunks_min=32, exact="none"))
    # alignment pass, every route once (first the 15-state model at b = 3, L = 37)
    for names, b, L, expect in ((("g15",), 3, 37, dict(exact="none")), (("d16",), 3, 37, dict(exact="none")),
                                (("g29",), 3, 37, dict(exact="none")), (("d32",), 3, 37, dict(exact="none")),
                                (("d64",), 2, 300, dict(scan64=True, exact="none")), (("g43",), 3, 37, dict(scan64=False)),
                                (("s67",), 65, 7, dict())):
        add(names, b, L, [], expect, tag="-odd", wrap=odd)
    # hmm_posterior without its optional log-likelihood
    for names, b, L, expect in ((("g15",), 3, 37, dict(exact="none")), (("g29",), 3, 37, dict(exact="none")),
                                (("g43",), 3, 37, dict(scan64=False)), (("s67",), 65, 7, dict())):
        add(names, b, L, [], expect, ops=REC_OPS[3:], tag="-no_ll", wrap=lambda build: build, no_ll=True)
    # the serial exact-clamp kernels: windows and whole sequences (AUTO on a zero stretch), every sequence (ALWAYS, NARROW)
    # (a row of zeros is a uniform emission floor: it moves no posterior, and nothing is born at a clamp.  The compiled
    # sparse reduce marks the chunk all the same, its columns pass through the denormal range between two rescales; the
    # dense reduce rescales every step and the certificate stays at zero: that row runs the routing kernels, flags nothing)
    for names, want in ((("g15",), "some"), (("d7",), "none"), (("d16",), "none")):
        add(names, 3, 100, [(C, 16), (X, engine.EXACT_AUTO)], dict(chunk=16, exact=want), stretch=True, tag="-zeros")
        for how in (engine.EXACT_ALWAYS, engine.EXACT_ALWAYS_NARROW):
            add(names, 3, 37, [(X, how)], dict(exact="all"))
    # ... two models of 17 sequences: waves of 16 sequences straddle the models, and the exact plan's checkpoints
    # (make_xplan: one chunk of ceil(L/16)*16 steps per sequence, one sequence per wave under NARROW) lie in the region
    # sized for the scan plan's
    for how in (engine.EXACT_ALWAYS, engine.EXACT_ALWAYS_NARROW):
        add(("g15", "d15"), 17, 100, [(C, 16), (X, how)], dict(chunk=16, exact="all"))
    # 17..32 states: rows of 32 lanes, the compiled 29-state reduce and the dense one
    for names, dense in ((("g29",), (0, 1)), (("d32",), (0,))):
        for fd in dense:
            add(names, 3, 37, [(D, fd)], dict(exact="none"))
            add(names, 17, 100, [(C, 16), (D, fd)], dict(exact="none"))
            add(names, 2, 530, [(C, 16), (D, fd)], dict(exact="none"))
    add(("g29",), 3, 100, [(C, 16)], dict(exact="some"), stretch=True, tag="-zeros")
    # 33..64 states: rows of 64 lanes for few long sequences, else one wave per sequence (hmm_midq.inc)
    for names in (("g43",), ("d64",)):
        add(names, 2, 300, [(C, 16)], dict(scan64=True, exact="none"))
        add(names, 3, 37, [], dict(scan64=False))
    # above 64 states: GEMM tiles, the helper stream
    for names in (("s67",), ("d129",)):
        add(names, 65, 7, [], dict())
    return out


# ---- Viterbi --------------------------------------------------------------------------------------------------------
def vit_build(symbol, names, b, L, expect):
    def build():
        lib = engine.lib()
        k, q = len(names), int(names[0][1:])
        logA, logpi = log_model(names)
        logE = np.log(emissions((symbol, names), k, b, L, q)).astype(np.float32)
        dims = (k, b, L, q)
        logA, logpi, logE = t32(logA), t32(logpi), t32(logE)
        args = [mc.Arg("A", "inp", logA), mc.Arg("pi", "inp", logpi), mc.Arg("E", "inp", logE, big=True),
                mc.Arg("path", "out", shape=(k, b, L), dtype=I32, big=True), mc.Arg("score", "out", shape=(k, b), dtype=F64),
                ws_arg(symbol + "_workspace_bytes", *dims)]
        argv = [Ref("A"), Ref("pi"), Ref("E"), *dims, Ref("path"), Ref("score"), Ref("ws"), Bytes("ws"), STREAM]
        fn = getattr(engine, symbol[4:])
        wrapper = lambda: dict(zip(("path", "score"), fn(dev(logA), dev(logpi), dev(logE))))

        def route(rep):
            if symbol == "hmm_viterbi":
                assert q <= lib.hmm_viterbi_max_states()
                assert q > 16 or (L + lib.hmm_chunk_len(*dims) - 1) // lib.hmm_chunk_len(*dims) >= expect.get("chunks_min", 1)
                assert q <= 16 or not lib.hmm_viterbi_scan_pays(*dims)       # (engine.viterbi, the wrapper of P, stays here)
            elif symbol == "hmm_viterbi_scan":
                T = lib.hmm_viterbi_scan_chunk_len(*dims)
                assert 0 < T and (L + T - 1) // T >= expect.get("chunks_min", 2), T
            else:
                assert engine.get_option(engine.OPT_VLARGE) in (1, 2) and q <= (1024 if engine.get_option(engine.OPT_VLARGE) == 1 else 4096)

        return mc.Spec(symbol, expect.get("label", "walk"), args, wrapper=wrapper), c_call(symbol, argv), route
    return build


def viterbi_rows():
    out = []
    C, S2, G, D = engine.OPT_CHUNK, engine.OPT_SCAN2, engine.OPT_VGROUPS, engine.OPT_FORCE_DENSE

    def add(symbol, name, b, L, options, expect):
        out.append(Row("%s-%s-b%d-L%d%s" % (symbol[4:], name, b, L, opt_id(options)), symbol,
                       vit_build(symbol, (name,), b, L, expect), options))

    for name in ("g15", "d7", "d16", "g29", "d40"):
        add("hmm_viterbi", name, 3, 37, [], dict())
        for two in (1, 0):
            add("hmm_viterbi", name, 2, 530, [(C, 16), (S2, two)], dict(chunks_min=32))
        for groups in (1, 3):
            add("hmm_viterbi", name, 70, 37, [(G, groups)], dict())
    add("hmm_viterbi", "g15", 3, 37, [(D, 1)], dict())
    add("hmm_viterbi", "g29", 3, 37, [(D, 1)], dict())
    for name in ("g29", "d64"):
        add("hmm_viterbi_scan", name, 2, 100, [(C, 16)], dict(chunks_min=7, label="scan"))
        for two in (1, 0):
            add("hmm_viterbi_scan", name, 2, 530, [(C, 16), (S2, two)], dict(chunks_min=32, label="scan"))
    add("hmm_viterbi_scan", "g29", 2, 530, [(C, 16), (D, 1)], dict(chunks_min=32, label="scan"))
    for symbol, name, b, L, options in (("hmm_viterbi", "g15", 3, 37, []), ("hmm_viterbi", "d16", 2, 530, [(C, 16)]),
                                        ("hmm_viterbi", "g29", 3, 37, []), ("hmm_viterbi", "d40", 70, 37, [(G, 3)]),
                                        ("hmm_viterbi_scan", "g29", 2, 100, [(C, 16)]), ("hmm_viterbi_scan", "d64", 2, 100, [(C, 16)]),
                                        ("hmm_viterbi_large", "s71", 3, 37, [(engine.OPT_VLARGE, 1)]),
                                        ("hmm_viterbi_large", "d257", 65, 7, [(engine.OPT_VLARGE, 2)])):      # alignment pass
        out.append(Row("%s-%s-b%d-L%d%s-odd" % (symbol[4:], name, b, L, opt_id(options)), symbol,
                       odd(vit_build(symbol, (name,), b, L, dict(chunks_min=2 if "scan" in symbol else 1))), options))
    for name in ("s71", "d257"):
        for how in (1, 2):
            add("hmm_viterbi_large", name, 3, 37, [(engine.OPT_VLARGE, how)], dict(label="walk" if how == 1 else "tiles"))
            add("hmm_viterbi_large", name, 65, 7, [(engine.OPT_VLARGE, how)], dict(label="walk" if how == 1 else "tiles"))
    return out


# ---- gradients ------------------------------------------------------------------------------------------------------
def grad_build(symbol, names, b, L, log, optional, stretch, expect):
    """symbol: hmm_loglik_grad[_scan|_large] (log = None) or hmm_posterior_grad[_scan|_large] (log = False / True).
    optional: pass the arguments the header allows to be NULL (grad_loglik, loglik)."""
    posterior = "posterior" in symbol

    def build():
        lib = engine.lib()
        k, q = len(names), int(names[0][1:])
        A, pi = models(names)
        E = emissions((symbol, names), k, b, L, q, stretch)
        dims = (k, b, L, q)
        rng = rng_of("G", symbol, names, b, L)
        A, pi, E = t32(A), t32(pi), t32(E)
        args = [mc.Arg("A", "inp", A), mc.Arg("pi", "inp", pi), mc.Arg("E", "inp", E, big=True),
                mc.Arg("dA", "out", shape=(k, q, q)), mc.Arg("dpi", "out", shape=(k, q)),
                mc.Arg("dE", "out", shape=dims, big=True), ws_arg(symbol + "_workspace_bytes", *dims)]
        fn = getattr(engine, symbol[4:])
        if posterior:
            if log:
                # -1 on the most probable state (a cross-entropy on labels).  A dense upstream gradient in log mode is
                # exposed to the floors wherever a posterior is tiny and sends sequences to the sweeps by a rule that
                # depends on the draw (PC_LOG_EXPOSED); on labels the exposed weight is F / gamma_max, far below it
                from oracle import textbook
                Gn = np.stack([-(g == g.max(-1, keepdims=True)).astype(np.float32)
                               for g in (textbook.posterior(A[m].numpy().astype(np.float64), pi[m].numpy().astype(np.float64),
                                                            E[m].numpy().astype(np.float64))[0] for m in range(k))])
                G = t32(Gn)
            else:
                G = t32(rng.standard_normal(dims))
            mode = engine.POST_LOG if log else engine.POST_PROB
            args.append(mc.Arg("G", "inp", G, big=True))
            argv = [Ref("A"), Ref("pi"), Ref("E"), *dims, engine.EPS, mode, Ref("G"), Ref("dA"), Ref("dpi"), Ref("dE"),
                    Ref("ws"), Bytes("ws"), STREAM]
            wrapper = lambda: dict(zip(("dA", "dpi", "dE"), fn(dev(A), dev(pi), dev(E), dev(G), mode=mode)))
        else:
            w = t32(rng.random((k, b)) + 0.5)
            if optional:
                args += [mc.Arg("w", "inp", w), mc.Arg("ll", "out", shape=(k, b), dtype=F64)]
            argv = [Ref("A"), Ref("pi"), Ref("E"), *dims, engine.EPS, Ref("w"), Ref("dA"), Ref("dpi"), Ref("dE"), Ref("ll"),
                    Ref("ws"), Bytes("ws"), STREAM]

            def wrapper():
                res = dict(zip(("dA", "dpi", "dE", "ll"), fn(dev(A), dev(pi), dev(E), dev(w) if optional else None)))
                if not optional:
                    del res["ll"]
                return res
        reader = None if symbol.endswith("_large") else symbol + "_serial_count"

        def diag(arena):
            n = getattr(lib, reader)(*dims, arena.ptr("ws"), arena.nbytes("ws"))
            assert n >= 0, n
            return (int(n),)

        def route(rep):
            stem = symbol[:-len("_scan")] if symbol.endswith("_scan") else symbol
            if symbol.endswith("_scan") and q > 16:
                T = getattr(lib, symbol + "_chunk_len")(*dims)
                assert 0 < T < L, T                           # more than one chunk
            if not symbol.endswith("_scan") and not symbol.endswith("_large") and q > 16:
                assert not getattr(lib, symbol + "_scan_pays")(*dims)       # (the wrapper of P stays on this entry point)
            if symbol.endswith("_large"):
                assert engine.get_option(engine.OPT_GLARGE) in (1, 2)
                return
            n, want = rep.diag[0], expect
            assert want is None or (n == 0 if want == "none" else n == k * b if want == "all" else 0 < n < k * b), \
                (stem, n, want)

        spec = mc.Spec(symbol, "%s%s" % (expect or "by-q", "" if log is None else "-log" if log else "-prob"), args,
                       wrapper=wrapper, diag=diag if reader else None)
        return spec, c_call(symbol, argv), route
    return build


def grad_rows():
    out = []
    C, PG, GL = engine.OPT_CHUNK, engine.OPT_PGCHUNK, engine.OPT_GLARGE

    def add(symbol, name, b, L, log, optional, options, expect, stretch=False):
        tag = "" if log is None else "-log" if log else "-prob"
        out.append(Row("%s-%s-b%d-L%d%s%s%s%s" % (symbol[4:], name, b, L, tag, "-opt" if optional else "",
                                                  "-zeros" if stretch else "", opt_id(options)), symbol,
                       grad_build(symbol, (name,), b, L, log, optional, stretch, expect), options))

    # header: hmm_loglik_grad serves 17..64 states by whole-sequence sweeps, except the compiled 29-state topology
    # (per chunk; OPT_PGCHUNK = 0 sends it to the sweeps too); up to 16 states the count is hmm_exact_count's
    for name, per_chunk in (("g15", True), ("g29", True), ("g57", False)):
        for how in (0, 1, 2):
            want = "none" if per_chunk and (how or name == "g15") else "all"
            for optional in (False, True):
                add("hmm_loglik_grad", name, 3, 100, None, optional, [(C, 16), (PG, how)], want)
    add("hmm_loglik_grad", "g15", 3, 100, None, True, [(C, 16)], "some", stretch=True)
    # (the 29-state path of hmm_loglik_grad runs without the reduce's marks: only the certificate F flags, and a uniform
    # floor leaves it at zero — hence the stretch in which one single-successor state alone emits)
    add("hmm_loglik_grad", "g29", 3, 100, None, True, [(C, 16)], "some", stretch="only")
    for name in ("g15", "g29", "g57", "d32"):
        for optional in (False, True):
            add("hmm_loglik_grad_scan", name, 3, 100, None, optional, [(C, 16)], "none")
    add("hmm_loglik_grad_scan", "g57", 3, 100, None, True, [(C, 16), (PG, 2)], "none")
    add("hmm_loglik_grad_scan", "g57", 3, 100, None, True, [(C, 16)], "some", stretch=True)
    for name in ("g15", "g29", "g57", "d80"):
        for how in (1, 2):
            for optional in (False, True):
                add("hmm_loglik_grad_large", name, 3, 37, None, optional, [(GL, how)], None)
    add("hmm_loglik_grad_large", "d80", 65, 7, None, True, [(GL, 2)], None)
    # posterior gradients: OPT_PGCHUNK 0 = whole-sequence sweeps, 2 = every sequence per chunk where the model is
    # eligible (up to 16 states, the compiled 29-state topology), 1 = where it pays (pc_wanted: up to 4096 sequences
    # of up to 16 states, 512 of the 29-state model, from four chunks on — 3 sequences of 7 chunks here) under the
    # certificate, which these inputs pass: per chunk as well
    for name, per_chunk in (("g15", True), ("g29", True), ("g57", False)):
        for log in (False, True):
            for how, want in ((0, "all"), (1, "none" if per_chunk else "all"), (2, "none" if per_chunk else "all")):
                # (57 states at L = 37: below the four chunks from which hmm_posterior_grad_scan_pays hands the
                # wrapper's call to hmm_posterior_grad_scan)
                add("hmm_posterior_grad", name, 3, 100 if per_chunk else 37, log, False, [(C, 16), (PG, how)], want)
    # one clamp-routed sequence: the whole-sequence sweeps redo it beside the per-chunk evaluation of the other two
    for name in ("g15", "g29"):
        for log in (False, True):
            add("hmm_posterior_grad", name, 3, 100, log, False, [(C, 16), (PG, 1)], "some", stretch="only")
    for name in ("g15", "g29", "g57", "d32"):
        for log in (False, True):
            add("hmm_posterior_grad_scan", name, 3, 100, log, False, [(C, 16), (PG, 2)], "none")
    add("hmm_posterior_grad_scan", "g57", 3, 100, False, False, [(C, 16)], "none")         # under the certificate
    add("hmm_posterior_grad_scan", "g57", 3, 100, False, False, [(C, 16)], "some", stretch=True)
    add("hmm_posterior_grad_scan", "g29", 3, 100, True, False, [(C, 16)], "some", stretch=True)
    for name in ("g15", "g29", "g57", "d80"):
        for how in (1, 2):
            for log in (False, True):
                add("hmm_posterior_grad_large", name, 3, 37, log, False, [(GL, how)], None)
    add("hmm_posterior_grad_large", "d80", 65, 7, False, False, [(GL, 2)], None)
    # alignment pass: every entry point, per chunk and by whole-sequence sweeps, walk and GEMMs
    for symbol, name, L, log, options, want in (
            ("hmm_loglik_grad", "g15", 100, None, [(C, 16)], "none"), ("hmm_loglik_grad", "g29", 100, None, [(C, 16)], "none"),
            ("hmm_loglik_grad", "g57", 100, None, [(C, 16)], "all"), ("hmm_loglik_grad_scan", "g57", 100, None, [(C, 16)], "none"),
            ("hmm_loglik_grad_scan", "d32", 100, None, [(C, 16)], "none"),
            ("hmm_loglik_grad_large", "d80", 37, None, [(GL, 1)], None), ("hmm_loglik_grad_large", "d80", 37, None, [(GL, 2)], None),
            ("hmm_posterior_grad", "g15", 100, True, [(C, 16), (PG, 2)], "none"),
            ("hmm_posterior_grad", "g29", 100, False, [(C, 16), (PG, 2)], "none"),
            ("hmm_posterior_grad", "g57", 37, True, [(C, 16)], "all"),
            ("hmm_posterior_grad_scan", "g57", 100, True, [(C, 16), (PG, 2)], "none"),
            ("hmm_posterior_grad_scan", "d32", 100, False, [(C, 16), (PG, 2)], "none"),
            ("hmm_posterior_grad_large", "d80", 37, True, [(GL, 1)], None), ("hmm_posterior_grad_large", "d80", 37, False, [(GL, 2)], None)):
        tag = "" if log is None else "-log" if log else "-prob"
        out.append(Row("%s-%s-b3-L%d%s%s-odd" % (symbol[4:], name, L, tag, opt_id(options)), symbol,
                       odd(grad_build(symbol, (name,), 3, L, log, log is None, False, want)), options))
    return out


# ---- the gene emitter -----------------------------------------------------------------------------------------------
EMITTER_MODELS = {"default": (dict(), 15), "s7": (dict(), 7), "s20": (dict(), 20),
                  "copies2_unshared": (dict(num_copies=2, share_intron_parameters=False), 15),
                  "copies3": (dict(num_copies=3), 15)}
EMITTER_SHAPES = ((3, 5), (7, 16), (4, 37), (2, 1100))


@functools.lru_cache(maxsize=None)
def emitter_tables(name):
    from hmm_layer_amd.gene_pred_hmm_emitter import GenePredHMMEmitter
    kw, s = EMITTER_MODELS[name]
    em = GenePredHMMEmitter(**CODONS, **kw)
    em.build((1, 2, 5, s))
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    with torch.no_grad():
        em.emission_kernel.copy_(torch.randn(em.emission_kernel.shape, generator=g))
        B = em.make_B()[0].contiguous().float()
    row, cod = em.state_tables(torch.device("cpu"))
    return B, row.contiguous(), em.codon_probs.detach().float().contiguous(), cod.contiguous(), s


def class_and_nucleotides(key, b, L, s, soft):
    g = torch.Generator().manual_seed(zlib.crc32(repr((key, b, L, s, soft)).encode()))
    cls = torch.softmax(2 * torch.randn((b, L, s), generator=g), -1)
    nuc = torch.nn.functional.one_hot(torch.randint(0, 5, (b, L), generator=g), 5).float()
    if soft:
        kind = torch.rand((b, L), generator=g)
        nuc = torch.where((kind < 0.3)[..., None], torch.softmax(torch.randn((b, L, 5), generator=g), -1), nuc)
        nuc[..., 4] = torch.where((kind >= 0.3) & (kind < 0.4), torch.full_like(kind, 0.5), nuc[..., 4])
    return torch.cat([cls, nuc], -1).contiguous(), g


def gene_build(symbol, name, b, L, soft, want_dx=True, want_dB=True):
    grad = "_grad" in symbol

    def build():
        B, row, codon, cod, s = emitter_tables(name)
        rows, q, nc = B.shape[0], row.numel(), codon.shape[1]
        x, g = class_and_nucleotides(symbol, b, L, s, soft)
        free, add, n_mass = 1.0 / 4096.0, 1e-7, 1
        args = [mc.Arg("x", "inp", x, big=True), mc.Arg("B", "inp", B), mc.Arg("row", "inp", row),
                mc.Arg("codon", "inp", codon), mc.Arg("cod", "inp", cod)]
        head = [Ref("x"), b, L, s, Ref("B"), rows, Ref("row"), Ref("codon"), nc, Ref("cod"), q, free, add, n_mass]
        fn = getattr(engine, symbol[4:])
        tabs = lambda: (dev(x), dev(B), dev(row), dev(codon), dev(cod))
        if not grad:
            args.append(mc.Arg("E", "out", shape=(b, L, q), big=True))
            argv = head + [Ref("E"), STREAM]
            wrapper = lambda: dict(E=fn(*tabs(), free_value=free, add=add, n_mass=n_mass))
        else:
            dE = torch.randn((b, L, q), generator=g)
            args.append(mc.Arg("dE", "inp", dE, big=True))
            if want_dx:
                args.append(mc.Arg("dx", "out", shape=tuple(x.shape), big=True))
            if want_dB:
                args.append(mc.Arg("dB", "out", shape=tuple(B.shape)))
            args.append(ws_arg(symbol + "_workspace_bytes", b, L, s, rows, q))
            argv = head + [Ref("dE"), Ref("dx"), Ref("dB"), Ref("ws"), Bytes("ws"), STREAM]

            def wrapper():
                dx, dB = fn(*tabs(), dev(dE), free_value=free, add=add, n_mass=n_mass, want_dx=want_dx, want_dB=want_dB)
                return {n: v for n, v in (("dx", dx), ("dB", dB)) if v is not None}

        def route(rep):
            wide = engine.gene_emissions_routes_wide(q, rows)
            assert wide is not None and (("_wide" in symbol) or wide is False)

        return mc.Spec(symbol, "soft" if soft else "one-hot", args, wrapper=wrapper), c_call(symbol, argv), route
    return build


def gene_rows():
    out = []

    def add(symbol, name, b, L, soft, **kw):
        tag = "".join("-no_%s" % n[5:] for n, v in kw.items() if not v)
        out.append(Row("%s-%s-b%d-L%d-%s%s" % (symbol[4:], name, b, L, "soft" if soft else "onehot", tag), symbol,
                       gene_build(symbol, name, b, L, soft, **kw)))

    narrow = ("default", "s7", "s20", "copies2_unshared")
    for fwd, bwd, names in (("hmm_gene_emissions", "hmm_gene_emissions_grad", narrow),
                            ("hmm_gene_emissions_wide", "hmm_gene_emissions_grad_wide", narrow + ("copies3",))):
        for name in names:
            for b, L in EMITTER_SHAPES:
                for soft in (False, True):
                    add(fwd, name, b, L, soft)
                add(bwd, name, b, L, (b + L) % 2 == 1)
            add(bwd, name, 4, 37, True, want_dB=False)
            add(bwd, name, 4, 37, True, want_dx=False)
            add(bwd, name, 2, 1100, False, want_dx=False)
        # alignment pass.  em_flush_flat stores whole tiles as aligned 16-byte pieces: E of the narrow forward and dx of
        # both backwards need 16 bytes and stay aligned; the wide forward stores 4-byte-aligned vectors
        keep = ("dx",) if "wide" in fwd else ("E", "dx")
        for name in names[:1] + names[-1:]:
            for symbol in (fwd, bwd):
                out.append(Row("%s-%s-b4-L37-soft-odd" % (symbol[4:], name), symbol,
                               odd(gene_build(symbol, name, 4, 37, True), keep)))
    return out


# ---- the embedding emitter -------------------------------------------------------------------------------------------
DMAX = 4096             # hmm_embedding_emissions_max_dim(); the rows at d = DMAX assert that it still is (no library here)
EMB_ROWMAPS = {"q15": (13, [0, 1, 1, 1] + list(range(2, 13))),
               "q43": (37, [0, 1, 2, 3, 1, 2, 3] + list(range(4, 37)) + [40, -2, 36])}      # two entries are clamped


def embedding_build(symbol, rowmap, b, L, d, s, multiply, outputs=("dE_in", "demb", "tables"), in_place=True):
    """x (b, L, s + d + 5) with the embedding in columns s .. s+d-1 (ld > d, col0 > 0) unless s is None (ld = d).
    The other columns belong to the window, not to the argument: they are filled like a margin (R1).  demb goes into
    the same columns of a (b, L, s + d + 5) output whose other columns must stay (W1), or, in_place = False, into a
    (b, L, d) tensor."""
    grad = "_grad" in symbol

    def build():
        rows, state_row = EMB_ROWMAPS[rowmap]
        q = len(state_row)
        g = torch.Generator().manual_seed(zlib.crc32(repr((symbol, rowmap, b, L, d)).encode()))
        mean = torch.randn((rows, d), generator=g)
        sigma = (0.8 + 0.4 * torch.rand((rows, d), generator=g)).double()
        inv_std = (1.0 / sigma).float()
        log_norm = (-0.5 * d * np.log(2 * np.pi) - sigma.log().sum(-1)).float()
        col0, w = (0, d) if s is None else (s, s + d + 5)
        x = torch.randn((b, L, w), generator=g)
        inside = torch.zeros((b, L, w), dtype=torch.bool)
        inside[..., col0:col0 + d] = True
        mask = None if s is None else inside
        row = torch.tensor(state_row, dtype=I32)
        T = 1.0 / max(1.0, d / 8.0)                               # inv_temperature: keeps exp() in range for wide embeddings
        add = 1e-7
        Ein = (0.5 + torch.rand((b, L, q), generator=g)).contiguous()
        args = [mc.Arg("x", "inp", x, big=True, mask=mask), mc.Arg("mean", "inp", mean), mc.Arg("inv_std", "inp", inv_std),
                mc.Arg("log_norm", "inp", log_norm), mc.Arg("row", "inp", row)]
        head = [Ref("x", 4 * col0), w, b, L, d, Ref("mean"), Ref("inv_std"), Ref("log_norm"), rows, Ref("row"), q, T, add]
        fn = getattr(engine, symbol[4:])
        tabs = lambda: (dev(x), col0, d, dev(mean), dev(inv_std), dev(log_norm), dev(row))
        if not grad:
            args.append(mc.Arg("E", "inout", Ein, big=True) if multiply
                        else mc.Arg("E", "out", shape=(b, L, q), big=True))
            argv = head + [multiply, Ref("E"), STREAM]
            wrapper = lambda: dict(E=fn(*tabs(), E=dev(Ein).clone() if multiply else None, inv_temperature=T, add=add))
        else:
            dE = torch.randn((b, L, q), generator=g)
            args.append(mc.Arg("dE", "inp", dE, big=True))
            if multiply:
                args.append(mc.Arg("Ein", "inp", Ein, big=True))
            want_dE_in = multiply and "dE_in" in outputs
            if want_dE_in:
                args.append(mc.Arg("dE_in", "out", shape=(b, L, q), big=True))
            ldd, off = 0, 0
            if "demb" in outputs:
                if in_place and s is not None:
                    args.append(mc.Arg("demb", "out", shape=(b, L, w), big=True, mask=inside))
                    ldd, off = w, 4 * col0
                else:
                    args.append(mc.Arg("demb", "out", shape=(b, L, d), big=True))
                    ldd = d
            if "tables" in outputs:
                args += [mc.Arg("dmean", "out", shape=(rows, d)), mc.Arg("dinv_std", "out", shape=(rows, d)),
                         mc.Arg("dlog_norm", "out", shape=(rows,))]
            args.append(ws_arg(symbol + "_workspace_bytes", b, L, d, rows, q))
            argv = head + [Ref("Ein"), Ref("dE"), Ref("dE_in"), Ref("demb", off), ldd, Ref("dmean"), Ref("dinv_std"),
                           Ref("dlog_norm"), Ref("ws"), Bytes("ws"), STREAM]

            def wrapper():
                dx_out = torch.zeros((b, L, w), device=DEV) if ldd == w and s is not None else None
                res = fn(*tabs(), dev(dE), E_in=dev(Ein) if multiply else None, inv_temperature=T, add=add,
                         want_dE_in=want_dE_in, want_demb="demb" in outputs, want_tables="tables" in outputs, dx_out=dx_out)
                return {n: v for n, v in zip(("dE_in", "demb", "dmean", "dinv_std", "dlog_norm"), res) if v is not None}

        def route(rep):
            wide = engine.embedding_emissions_routes_wide(q, rows)
            assert wide is not None and (("_wide" in symbol) or wide is False)
            dmax = engine.lib().hmm_embedding_emissions_max_dim()
            assert d <= dmax and (d != DMAX or d == dmax)       # the "d at its maximum" rows are at the maximum

        return mc.Spec(symbol, "multiply%d" % multiply, args, wrapper=wrapper), c_call(symbol, argv), route
    return build


def embedding_rows():
    out = []
    dmax = DMAX

    def add(symbol, rowmap, b, L, d, s, multiply, wrap=None, **kw):
        tag = "" if "outputs" not in kw else "-" + "+".join(kw["outputs"])
        tag += "" if kw.get("in_place", True) else "-packed"
        tag += "-odd" if wrap else ""
        build = embedding_build(symbol, rowmap, b, L, d, s, multiply, **kw)
        out.append(Row("%s-%s-b%d-L%d-d%d-%s-m%d%s" % (symbol[4:], rowmap, b, L, d, "ld%d" % d if s is None else "col%d" % s,
                                                      multiply, tag), symbol, wrap(build) if wrap else build))

    for fwd, bwd, maps in (("hmm_embedding_emissions", "hmm_embedding_emissions_grad", ("q15",)),
                           ("hmm_embedding_emissions_wide", "hmm_embedding_emissions_grad_wide", ("q15", "q43"))):
        for rowmap in maps:
            for multiply in (0, 1):
                for b, L, d, s in ((4, 37, 17, 15), (2, 1100, 16, 15), (7, 16, 1, 15), (3, 5, dmax, 15), (4, 37, 3, None)):
                    add(fwd, rowmap, b, L, d, s, multiply)
                    add(bwd, rowmap, b, L, d, s, multiply)
            add(bwd, rowmap, 4, 37, 17, 15, 1, outputs=("demb",))
            add(bwd, rowmap, 4, 37, 17, 15, 1, outputs=("demb",), in_place=False)
            add(bwd, rowmap, 4, 37, 17, 15, 1, outputs=("tables",))
            add(bwd, rowmap, 2, 1100, 16, 15, 1, outputs=("dE_in",))
            for multiply in (0, 1):                              # alignment pass
                add(fwd, rowmap, 4, 37, 17, 15, multiply, wrap=odd)
            add(bwd, rowmap, 4, 37, 17, 15, 1, wrap=odd)
            add(bwd, rowmap, 4, 37, 17, 15, 1, in_place=False, wrap=odd)
    return out


# ---- the nucleotide emitter ------------------------------------------------------------------------------------------
def gene_map(c):
    return [j - (1 + 3 * c) if 1 + 3 * c <= j < 1 + 6 * c else -1 for j in range(1 + 14 * c)]


NUC_ROWMAPS = {15: (3, gene_map(1)), 29: (6, gene_map(2)), 256: (256, list(range(256)))}


def nucleotide_build(symbol, q, ld, b, L, multiply, outputs=("dE_in", "dP")):
    grad = "_grad" in symbol

    def build():
        rows, state_nuc = NUC_ROWMAPS[q]
        g = torch.Generator().manual_seed(zlib.crc32(repr((symbol, q, ld, b, L)).encode()))
        nuc = torch.nn.functional.one_hot(torch.randint(0, 5, (b, L), generator=g), 5).float()
        kind = torch.rand((b, L), generator=g)
        nuc = torch.where((kind < 0.3)[..., None], torch.softmax(torch.randn((b, L, 5), generator=g), -1), nuc)
        nuc = torch.where((kind >= 0.9)[..., None], torch.zeros_like(nuc), nuc)
        col0 = ld - 5
        x = torch.randn((b, L, ld), generator=g)
        x[..., col0:] = nuc
        mask = None
        if col0:
            mask = torch.zeros((b, L, ld), dtype=torch.bool)
            mask[..., col0:] = True
        P = torch.softmax(torch.randn((rows, 4), generator=g), -1)
        tab = torch.tensor(state_nuc, dtype=I32)
        Ein = 0.5 + torch.rand((b, L, q), generator=g)
        args = [mc.Arg("x", "inp", x, big=True, mask=mask), mc.Arg("P", "inp", P), mc.Arg("tab", "inp", tab)]
        head = [Ref("x", 4 * col0), ld, b, L, Ref("P"), rows, Ref("tab"), q, 0.25]
        if not grad:
            args.append(mc.Arg("E", "inout", Ein, big=True) if multiply
                        else mc.Arg("E", "out", shape=(b, L, q), big=True))
            argv = head + [multiply, Ref("E"), STREAM]
            wrapper = lambda: dict(E=engine.nucleotide_emissions(dev(x), col0, dev(P), dev(tab),
                                                                 E=dev(Ein).clone() if multiply else None))
        else:
            dE = torch.randn((b, L, q), generator=g)
            args.append(mc.Arg("dE", "inp", dE, big=True))
            if multiply:
                args.append(mc.Arg("Ein", "inp", Ein, big=True))
            if "dE_in" in outputs:
                args.append(mc.Arg("dE_in", "out", shape=(b, L, q), big=True))
            if "dP" in outputs:
                args.append(mc.Arg("dP", "out", shape=(rows, 4)))
            args.append(ws_arg(symbol + "_workspace_bytes", b, L, rows, q))
            argv = head + [Ref("Ein"), Ref("dE"), Ref("dE_in"), Ref("dP"), Ref("ws"), Bytes("ws"), STREAM]

            def wrapper():
                res = engine.nucleotide_emissions_grad(dev(x), col0, dev(P), dev(tab), dev(dE), E_in=dev(Ein) if multiply else None,
                                                       want_dE_in="dE_in" in outputs, want_dP="dP" in outputs)
                return {n: v for n, v in zip(("dE_in", "dP"), res) if v is not None}

        def route(rep):
            assert q <= engine.lib().hmm_nucleotide_emissions_max_states()

        return mc.Spec(symbol, "multiply%d-ld%d" % (multiply, ld), args, wrapper=wrapper), c_call(symbol, argv), route
    return build


def nucleotide_rows():
    out = []
    for q in (15, 29, 256):
        for ld in (5, 25):
            for b, L in ((3, 1), (4, 37), (7, 16)):
                for multiply in (0, 1):
                    for symbol in ("hmm_nucleotide_emissions", "hmm_nucleotide_emissions_grad"):
                        out.append(Row("%s-q%d-ld%d-b%d-L%d-m%d" % (symbol[4:], q, ld, b, L, multiply), symbol,
                                       nucleotide_build(symbol, q, ld, b, L, multiply)))
        for symbol in ("hmm_nucleotide_emissions", "hmm_nucleotide_emissions_grad"):        # alignment pass
            out.append(Row("%s-q%d-ld25-b4-L37-m1-odd" % (symbol[4:], q), symbol,
                           odd(nucleotide_build(symbol, q, 25, 4, 37, 1))))
        for outputs in (("dE_in",), ("dP",)):
            out.append(Row("nucleotide_emissions_grad-q%d-ld25-b4-L37-m1-%s" % (q, outputs[0]), "hmm_nucleotide_emissions_grad",
                           nucleotide_build("hmm_nucleotide_emissions_grad", q, 25, 4, 37, 1, outputs)))
    return out


# ---- sequence-sharded calls: R = 3 slabs in turn on one device ---------------------------------------------------------
CUTS = (0, 33, 50, 100)


def lanes_below(q, *shape):
    m = torch.zeros(shape, dtype=torch.bool)
    m[..., :q] = True
    return m


def seqshard_build(name, mode, optional=True):
    """hmm_seqshard_reduce for every slab, the host's all-gather, hmm_seqshard_posterior for every slab.  Every slab has
    a workspace of its own (its chunk operators stay there between the two calls: that region is kept by design, so the
    pre-fill is applied before the first call of the sequence only); all margins are checked after every call.  The
    exponent lanes from q on carry no contract (header): they are left out of every comparison.  optional = False:
    without the outputs that may be NULL (loglik, phi_out)."""
    def build():
        lib = engine.lib()
        k, b, q, R = 1, 3, int(name[1:]), len(CUTS) - 1
        A, pi = models((name,))
        E = emissions(("seqshard", name), k, b, CUTS[-1], q)
        A, pi = t32(A), t32(pi)
        slabs = [t32(E[:, :, CUTS[r]:CUTS[r + 1]]) for r in range(R)]
        args = [mc.Arg("A", "inp", A), mc.Arg("pi", "inp", pi),
                mc.Arg("all_ops", "out", shape=(k, b, R, 16, 16)),
                mc.Arg("all_exps", "out", shape=(k, b, R, 16), dtype=I32, mask=lanes_below(q, k, b, R, 16), loose=True)]
        for r in range(R):
            Ls = CUTS[r + 1] - CUTS[r]
            args += [mc.Arg("E%d" % r, "inp", slabs[r], big=True), mc.Arg("op%d" % r, "out", shape=(k, b, 16, 16)),
                     mc.Arg("ex%d" % r, "out", shape=(k, b, 16), dtype=I32, mask=lanes_below(q, k, b, 16), loose=True),
                     mc.Arg("out%d" % r, "out", shape=(k, b, Ls, q), big=True),
                     ws_arg("hmm_seqshard_workspace_bytes", k, b, Ls, q, R, name="ws%d" % r)]
            if optional:
                args += [mc.Arg("ll%d" % r, "out", shape=(k, b), dtype=F64), mc.Arg("phi%d" % r, "out", shape=(k, b))]

        def call(arena):
            for r in range(R):
                Ls = CUTS[r + 1] - CUTS[r]
                invoke(arena, "hmm_seqshard_reduce", [Ref("A"), Ref("E%d" % r), k, b, Ls, q, engine.EPS, int(r == 0), R,
                                                      Ref("op%d" % r), Ref("ex%d" % r), Ref("ws%d" % r), Bytes("ws%d" % r), STREAM])
                arena.check("hmm_seqshard_reduce of slab %d" % r)
            for r in range(R):
                arena.view("all_ops")[:, :, r].copy_(arena.view("op%d" % r))
                arena.view("all_exps")[:, :, r].copy_(arena.view("ex%d" % r))
            for r in range(R):
                Ls = CUTS[r + 1] - CUTS[r]
                invoke(arena, "hmm_seqshard_posterior", [Ref("A"), Ref("pi"), Ref("E%d" % r), k, b, Ls, q, engine.EPS, int(r == 0),
                                                         Ref("all_ops"), Ref("all_exps"), R, r, mode, Ref("out%d" % r),
                                                         Ref("ll%d" % r), Ref("phi%d" % r), Ref("ws%d" % r), Bytes("ws%d" % r), STREAM])
                arena.check("hmm_seqshard_posterior of slab %d" % r)

        def wrapper():
            streams = [torch.cuda.Stream() for _ in range(R)]        # one cached workspace per stream = per slab
            res, red = {}, []
            torch.cuda.synchronize()
            for r in range(R):
                with torch.cuda.stream(streams[r]):
                    red.append(engine.seqshard_reduce(dev(A), dev(slabs[r]), r == 0, R))
            torch.cuda.synchronize()
            all_ops = torch.stack([o for o, _ in red], dim=2).contiguous()
            all_exps = torch.stack([e for _, e in red], dim=2).contiguous()
            torch.cuda.synchronize()
            for r in range(R):
                with torch.cuda.stream(streams[r]):
                    o, ll, phi = engine.seqshard_posterior(dev(A), dev(pi), dev(slabs[r]), all_ops, all_exps, r, mode)
                res.update({"op%d" % r: red[r][0], "ex%d" % r: red[r][1], "out%d" % r: o, "ll%d" % r: ll, "phi%d" % r: phi})
            torch.cuda.synchronize()
            return res if optional else {n: v for n, v in res.items() if n[:2] not in ("ll", "ph")}

        def route(rep):
            assert q <= lib.hmm_scan_max_states() and lib.hmm_chunk_len(k, b, CUTS[1], q) == 16
            if optional:                                              # the scan serves every sequence
                assert all(float(rep.outputs["phi%d" % r].max()) <= 1e-6 for r in range(R))

        spec = mc.Spec(("hmm_seqshard_reduce", "hmm_seqshard_posterior"), "R3-mode%d" % mode, args, wrapper=wrapper,
                       intermediate=("all_ops", "all_exps"), note="workspace pre-fill before the first call only")
        return spec, call, route
    return build


def seqshard_viterbi_build(name):
    """reduce, apply and path for every slab, the host's two all-gathers in between; workspaces and pre-fill as for
    seqshard_build.  Lanes from q on of vbase and origin are left out of the comparisons (the header defines the leading
    q entries)."""
    def build():
        lib = engine.lib()
        k, b, q, R = 1, 3, int(name[1:]), len(CUTS) - 1
        logA, logpi = log_model((name,))
        logE = np.log(emissions(("seqshard_viterbi", name), k, b, CUTS[-1], q)).astype(np.float32)
        logA, logpi = t32(logA), t32(logpi)
        slabs = [t32(logE[:, :, CUTS[r]:CUTS[r + 1]]) for r in range(R)]
        args = [mc.Arg("A", "inp", logA), mc.Arg("pi", "inp", logpi),
                mc.Arg("all_vops", "out", shape=(k, b, R, 16, 16), dtype=I32),
                mc.Arg("all_vbases", "out", shape=(k, b, R, 16), dtype=I64, mask=lanes_below(q, k, b, R, 16), loose=True),
                mc.Arg("all_origins", "out", shape=(k, b, R, 16), dtype=U8, mask=lanes_below(q, k, b, R, 16), loose=True)]
        for r in range(R):
            Ls = CUTS[r + 1] - CUTS[r]
            args += [mc.Arg("E%d" % r, "inp", slabs[r], big=True), mc.Arg("vop%d" % r, "out", shape=(k, b, 16, 16), dtype=I32),
                     mc.Arg("vbase%d" % r, "out", shape=(k, b, 16), dtype=I64, mask=lanes_below(q, k, b, 16), loose=True),
                     mc.Arg("origin%d" % r, "out", shape=(k, b, 16), dtype=U8, mask=lanes_below(q, k, b, 16), loose=True),
                     mc.Arg("final%d" % r, "out", shape=(k, b), dtype=I32), mc.Arg("score%d" % r, "out", shape=(k, b), dtype=F64),
                     mc.Arg("path%d" % r, "out", shape=(k, b, Ls), dtype=I32, big=True),
                     ws_arg("hmm_seqshard_viterbi_workspace_bytes", k, b, Ls, q, R, name="ws%d" % r)]

        def call(arena):
            Ls = [CUTS[r + 1] - CUTS[r] for r in range(R)]
            for r in range(R):
                invoke(arena, "hmm_seqshard_viterbi_reduce", [Ref("A"), Ref("pi"), Ref("E%d" % r), k, b, Ls[r], q, int(r == 0), R,
                                                              Ref("vop%d" % r), Ref("vbase%d" % r), Ref("ws%d" % r),
                                                              Bytes("ws%d" % r), STREAM])
                arena.check("hmm_seqshard_viterbi_reduce of slab %d" % r)
            for r in range(R):
                arena.view("all_vops")[:, :, r].copy_(arena.view("vop%d" % r))
                arena.view("all_vbases")[:, :, r].copy_(arena.view("vbase%d" % r))
            for r in range(R):
                invoke(arena, "hmm_seqshard_viterbi_apply", [Ref("A"), Ref("pi"), Ref("E%d" % r), k, b, Ls[r], q, int(r == 0),
                                                             Ref("all_vops"), Ref("all_vbases"), R, r, Ref("origin%d" % r),
                                                             Ref("final%d" % r), Ref("score%d" % r), Ref("ws%d" % r),
                                                             Bytes("ws%d" % r), STREAM])
                arena.check("hmm_seqshard_viterbi_apply of slab %d" % r)
            for r in range(R):
                arena.view("all_origins")[:, :, r].copy_(arena.view("origin%d" % r))
            for r in range(R):
                invoke(arena, "hmm_seqshard_viterbi_path", [k, b, Ls[r], q, Ref("all_origins"), Ref("final%d" % r), R, r,
                                                            Ref("path%d" % r), Ref("ws%d" % r), Bytes("ws%d" % r), STREAM])
                arena.check("hmm_seqshard_viterbi_path of slab %d" % r)

        def wrapper():
            streams = [torch.cuda.Stream() for _ in range(R)]
            res = {}
            A_, pi_, E_ = dev(logA), dev(logpi), [dev(x) for x in slabs]
            torch.cuda.synchronize()
            red, app = [], []
            for r in range(R):
                with torch.cuda.stream(streams[r]):
                    red.append(engine.seqshard_viterbi_reduce(A_, pi_, E_[r], r == 0, R))
            torch.cuda.synchronize()
            all_vops = torch.stack([v for v, _ in red], dim=2).contiguous()
            all_vbases = torch.stack([v for _, v in red], dim=2).contiguous()
            torch.cuda.synchronize()
            for r in range(R):
                with torch.cuda.stream(streams[r]):
                    app.append(engine.seqshard_viterbi_apply(A_, pi_, E_[r], all_vops, all_vbases, r))
            torch.cuda.synchronize()
            all_origins = torch.stack([o for o, _, _ in app], dim=2).contiguous()
            torch.cuda.synchronize()
            for r in range(R):
                with torch.cuda.stream(streams[r]):
                    path = engine.seqshard_viterbi_path(tuple(E_[r].shape), all_origins, app[r][1], r)
                res.update({"vop%d" % r: red[r][0], "vbase%d" % r: red[r][1], "origin%d" % r: app[r][0],
                            "final%d" % r: app[r][1], "score%d" % r: app[r][2], "path%d" % r: path})
            torch.cuda.synchronize()
            return res

        def route(rep):
            assert q <= lib.hmm_seqshard_viterbi_max_states()
            whole, _ = engine.viterbi(dev(logA), dev(logpi), dev(t32(logE)))      # the slabs' pieces are the whole path
            assert torch.equal(torch.cat([rep.outputs["path%d" % r] for r in range(R)], dim=2), whole)

        spec = mc.Spec(("hmm_seqshard_viterbi_reduce", "hmm_seqshard_viterbi_apply", "hmm_seqshard_viterbi_path"), "R3", args,
                       wrapper=wrapper, intermediate=("all_vops", "all_vbases", "all_origins"),
                       note="workspace pre-fill before the first call only")
        return spec, call, route
    return build


def seqshard_rows():
    out = []
    for name in ("g15", "d7", "d16"):
        for mode in (engine.POST_PROB, engine.POST_LOG, engine.POST_LOG_NO_LL):
            out.append(Row("seqshard-%s-mode%d" % (name, mode), ("hmm_seqshard_reduce", "hmm_seqshard_posterior"),
                           seqshard_build(name, mode), [(engine.OPT_CHUNK, 16)]))
        for fd in (0, 1):
            out.append(Row("seqshard_viterbi-%s-dense%d" % (name, fd),
                           ("hmm_seqshard_viterbi_reduce", "hmm_seqshard_viterbi_apply", "hmm_seqshard_viterbi_path"),
                           seqshard_viterbi_build(name), [(engine.OPT_CHUNK, 16), (engine.OPT_FORCE_DENSE, fd)]))
    out.append(Row("seqshard-g15-mode1-no_ll_phi", ("hmm_seqshard_reduce", "hmm_seqshard_posterior"),
                   seqshard_build("g15", engine.POST_LOG, optional=False), [(engine.OPT_CHUNK, 16)]))
    for name in ("g15", "d7"):                                   # alignment pass
        out.append(Row("seqshard-%s-mode0-odd" % name, ("hmm_seqshard_reduce", "hmm_seqshard_posterior"),
                       odd(seqshard_build(name, engine.POST_PROB), keep=("all_ops",)), [(engine.OPT_CHUNK, 16)]))
        out.append(Row("seqshard_viterbi-%s-odd" % name,
                       ("hmm_seqshard_viterbi_reduce", "hmm_seqshard_viterbi_apply", "hmm_seqshard_viterbi_path"),
                       odd(seqshard_viterbi_build(name), keep=("all_vops",)), [(engine.OPT_CHUNK, 16)]))
    return out


# ---- hmm_loglik_partials -----------------------------------------------------------------------------------------------
def partials_build(weights):
    def build():
        k, b = 2, 17
        rng = rng_of("partials")
        ll = torch.from_numpy(-100.0 * rng.random((k, b)))
        w = t32(rng.random((k, b)) + 0.5)
        args = [mc.Arg("ll", "inp", ll), mc.Arg("partial", "out", shape=(k, 2), dtype=F64)]
        if weights:
            args.append(mc.Arg("w", "inp", w))
        argv = [Ref("ll"), Ref("w"), k, b, Ref("partial"), STREAM]
        wrapper = lambda: dict(partial=engine.loglik_partials(dev(ll), dev(w) if weights else None))
        return mc.Spec("hmm_loglik_partials", "weights" if weights else "ones", args, wrapper=wrapper), \
            c_call("hmm_loglik_partials", argv), lambda rep: None
    return build


def partials_rows():
    return [Row("loglik_partials-%s" % ("weights" if w else "ones"), "hmm_loglik_partials", partials_build(w)) for w in (True, False)] \
        + [Row("loglik_partials-weights-odd", "hmm_loglik_partials", odd(partials_build(True)))]


@functools.lru_cache(maxsize=None)
def rows():
    return tuple(recursion_rows() + viterbi_rows() + grad_rows() + gene_rows() + embedding_rows() + nucleotide_rows()
                 + seqshard_rows() + partials_rows())
