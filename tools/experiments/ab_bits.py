"""Two builds of the engine in one process, compared bit for bit: the scan plan for up to 16 states, the chunked scan
for 17..64 states, and one case each on the one-wave-per-sequence path (48 states, short) and the GEMM path (100):
   python ab_bits.py OLD.so NEW.so
Every model x shape x chunk length x routing mode below runs through forward (log-likelihood alone and with log
alpha), backward, the three posterior modes and (up to 64 states) loglik_grad on both libraries; the raw bits of every
output and the number of sequences routed to the serial kernels must be equal.  Emissions are spread over six decades
with ~40 % exact zeros, so that the clamps and the certificates fire.  Exit status 1 on any difference, or when no case
of up to 16 states routed a sequence under the automatic routing."""
import os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from hmm_layer_amd import engine
from hmm_layer_amd.gene_pred_hmm_transitioner import GenePredMultiHMMTransitioner

dev = torch.device("cuda:0")
libs = [os.path.abspath(p) for p in sys.argv[1:3]]
rng = np.random.default_rng(0)


def dense(q):
    A = rng.random((q, q)).astype(np.float32) ** 3 + 1e-3
    return A / A.sum(-1, keepdims=True), np.full(q, 1 / q, dtype=np.float32)


def cyclic(q):                                   # a cycle with one self loop: primitive, the longest possible index
    A = np.roll(np.eye(q, dtype=np.float32), 1, axis=1)
    A[0, 0] = A[0, 1] = 0.5
    return A, np.full(q, 1 / q, dtype=np.float32)


def sparse_random(q):                            # the cycle above plus three random successors per state
    A = cyclic(q)[0]
    for i in range(q):
        A[i, rng.choice(q, 3, replace=False)] += rng.random(3).astype(np.float32)
    return A / A.sum(-1, keepdims=True), np.full(q, 1 / q, dtype=np.float32)


def gene(k):
    tr = GenePredMultiHMMTransitioner(k=k, initial_exon_len=200, initial_intron_len=4500, initial_ir_len=10000)
    with torch.no_grad():
        return tr.make_A()[0].numpy(), tr.make_initial_distribution().reshape(-1).numpy()


def gene7():
    from oracle import params
    ed = params.edges_simple()
    lg = params.init_logits(ed, 1)
    return params.dense_A(ed, np.where(lg == 0, 1e-30, lg), 7).numpy(), np.full(7, 1 / 7, dtype=np.float32)


MODELS16 = [("dense3", dense(3)), ("dense16", dense(16)), ("gene7", gene7()), ("gene15", gene(1)),
            ("cyclic16", cyclic(16))]
MODELS32 = [("dense17", dense(17)), ("dense24", dense(24)), ("gene29", gene(2)), ("dense32", dense(32)),
            ("cyclic32", cyclic(32))]
MODELS64 = [("dense33", dense(33)), ("gene43", gene(3)), ("gene57", gene(4)), ("dense64", dense(64)),
            ("sparse64", sparse_random(64))]
SHAPES32 = [(1, 1, 1), (1, 3, 17), (2, 5, 100), (1, 2, 1031)]
SHAPES64 = [(1, 2, 256), (2, 3, 1031), (1, 1, 4099)]          # (the 64-state rows serve L >= 256)
SHAPES16 = SHAPES32                                           # L = 1031, chunk 16: 65 chunks, the two-level chunk scan
AUTO_OFF = (engine.EXACT_AUTO, engine.EXACT_OFF)


def outputs(A, pi, E):
    """Every output of the entry points on this path, as integer tensors, and the routed-sequence counts."""
    dims = tuple(E.shape)
    res = {}
    res["loglik"] = engine.forward(A, pi, E, want_log_alpha=False)[1]
    res["n_loglik"] = engine.exact_count(engine.OP_LOGLIK, dims)
    res["log_alpha"], res["loglik_fw"] = engine.forward(A, pi, E)
    res["n_forward"] = engine.exact_count(engine.OP_FORWARD, dims)
    res["log_beta"] = engine.backward(A, E)
    res["n_backward"] = engine.exact_count(engine.OP_BACKWARD, dims)
    for mode in (engine.POST_PROB, engine.POST_LOG, engine.POST_LOG_NO_LL):
        res["post%d" % mode], res["post%d_ll" % mode] = engine.posterior(A, pi, E, mode=mode)
        res["n_post%d" % mode] = engine.exact_count(engine.OP_POSTERIOR, dims)
    if dims[3] <= 64:
        res["dA"], res["dpi"], res["dE"], res["grad_ll"] = engine.loglik_grad(A, pi, E)
        res["n_grad"] = engine.loglik_grad_serial_count(dims)
    return {k: v.view(torch.int32).clone() if torch.is_tensor(v) else v for k, v in res.items()}


bad = cases = 0
routed16 = 0                                  # q <= 16 cases under EXACT_AUTO with a non-zero routed count
for models, shapes, chunks, exacts in (
        (MODELS16, SHAPES16, (0, 16), AUTO_OFF + (engine.EXACT_ALWAYS,)),
        (MODELS32, SHAPES32, (0, 16), AUTO_OFF), (MODELS64, SHAPES64, (0, 16), AUTO_OFF),
        ([("dense48", dense(48))], [(1, 1, 100)], (0,), AUTO_OFF),       # one wave per sequence
        ([("dense100", dense(100))], [(1, 2, 40)], (0,), AUTO_OFF)):     # GEMM per step
    for name, (A1, pi1) in models:
        q = A1.shape[0]
        for k, b, L in shapes:
            A = torch.tensor(np.stack([A1] * k), device=dev)
            pi = torch.tensor(np.stack([pi1] * k), device=dev)
            E = (10.0 ** (-6 * rng.random((k, b, L, q)))).astype(np.float32)
            E[rng.random(E.shape) < 0.4] = 0.0
            E = torch.tensor(E, device=dev)
            for chunk in chunks:
                for exact in exacts:
                    got = []
                    for path in libs:
                        engine._lib = None; engine.LIB_PATH = path; engine.release_workspaces()
                        with engine.option(engine.OPT_CHUNK, chunk), engine.option(engine.OPT_EXACT, exact):
                            got.append(outputs(A, pi, E))
                    torch.cuda.synchronize()
                    diff = [key for key in got[0]
                            if not (torch.equal(got[0][key], got[1][key]) if torch.is_tensor(got[0][key])
                                    else got[0][key] == got[1][key])]
                    cases += 1
                    bad += bool(diff)
                    routed = {key: v for key, v in got[1].items() if key.startswith("n_")}
                    routed16 += q <= 16 and exact == engine.EXACT_AUTO and any(routed.values())
                    print("%-8s k=%d b=%d L=%-4d chunk=%-2d exact=%d  %s  routed %s" % (
                        name, k, b, L, chunk, exact, "DIFF " + ",".join(diff) if diff else "identical",
                        sorted(set(routed.values()))), flush=True)
print("%d cases, %d with a difference; %d cases of up to 16 states routed sequences under EXACT_AUTO" % (
    cases, bad, routed16))
sys.exit(1 if bad or not routed16 else 0)
