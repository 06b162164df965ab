"""Randomised parity sweep of hmm_forward / hmm_backward / hmm_posterior ABOVE 64 states (hmm_largeq.inc: one fused
f32-MFMA GEMM per position, the posterior's two recursions on two streams) against the fp64 serial recursion with the
cell's clamps (oracle/textbook.py).  tests/stress_sweep.py draws 1..64 states only; this one draws what that path has
boundaries in: state counts next to the 16-byte load, K-slab and tile-width boundaries, k = 1..3 models with ragged
batches, short and long sequences (the hand-over of the two recursions, the ping-pong of operands and partial sums),
degenerate models, and emissions with enough exact zeros that the parked product U_t * Rb_t underflows in fp32.

Test infrastructure.  draw_case(rng) does all the drawing and needs neither a GPU nor the engine;
tests/test_largeq_sweep_cpu.py asserts the coverage of the committed (N, seed) with it, tests/test_largeq_sweep_gpu.py
runs run(N, seed).  Case i of a seed has its own generator, case_rng(seed, i), so a failing case reruns alone:
    python tests/largeq_sweep.py [cases] [seed] [first case]

Tolerances (tests/test_engine_gpu.py, tests/test_scan32_gpu.py; restated here with the same numbers):
  posteriors          |gamma - gamma64| <= 2e-5; the log modes through exp at 2e-5 (POST_LOG_NO_LL: + 2.4e-7 max|ll64|)
                      and in log space at 1e-3 where gamma64 > 1e-4; rows of POST_PROB sum to 1 within 2e-5
  log alpha / beta    |x - x64| <= 3e-4 + 2e-7 |x64| where x64 > -30, and every component in probability space
  log-likelihood      |ll - ll64| <= 1e-6 |ll64| + 2e-4, bitwise the same from posterior, forward with and without log alpha
  k >= 2              every output bitwise equal to the k = 1 call on that model's slice
Log outputs may hold -inf where the fp32 product underflows (compared in probability space); NaN and +inf
never.  The -inf entries are counted and returned with the case.

The pool of (b, L) per case is cut so that k b L q <= ELEMS_MAX and k b L q^2 <= WORK_MAX (the fp64 oracle's memory
and time); no case is skipped and no check is switched off at run time."""
import os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
from oracle import textbook

N_CASES, SEED = 64, 239                # the committed sweep: search_seed(64), the first seed whose 64 shapes meet coverage()

Q_TRIPLES = [(65, 66, 67)] + [(n - 1, n, n + 1) for n in (96, 128, 160, 192, 256, 320, 512)]
Q_BOUNDARY = [q for tr in Q_TRIPLES for q in tr]
K_POOL = (1, 2, 3)
B_POOL = (1, 2, 63, 64, 65, 100, 129)
L_POOL = (1, 2, 5, 6, 64, 65, 400, 401)
L_LONG = (3000, 3001)
KINDS = ("dense", "sparse_diag", "ring", "block", "identity", "cycle", "zero_absorb", "gene5")
ZERO_FRACS = (0.0, 0.1, 0.3, 0.47)
ELEMS_MAX = 6.0e6                      # k b L q: each fp64 array of the oracle stays below 48 MB
WORK_MAX = 1.5e9                       # k b L q^2: a second or so of fp64 GEMMs per pass
GENE_LENGTHS = ((200, 4500, 10000), (50, 300, 900), (120, 1000, 3000))


def case_rng(seed, i):
    return np.random.default_rng([int(seed), int(i)])


def gene_model(copies, lengths=GENE_LENGTHS[0]):
    """A of the `copies`-copy gene model (1 + 14 copies states; five copies: the 71-state model of the README)."""
    import torch
    from hmm_layer_amd.gene_pred_hmm_transitioner import GenePredMultiHMMTransitioner
    tr = GenePredMultiHMMTransitioner(k=copies, initial_exon_len=lengths[0], initial_intron_len=lengths[1],
                                      initial_ir_len=lengths[2])
    with torch.no_grad():
        return tr.make_A()[0].numpy().astype(np.float32)


def draw_shape(rng):
    """The scalar part of a case (drawn first, so that coverage can be counted without building any array)."""
    kind = KINDS[int(rng.integers(0, len(KINDS)))]
    if kind == "gene5":
        q = 71
    elif rng.random() < 1 / 3:
        q = int(rng.integers(65, 601))
    else:
        q = int(Q_BOUNDARY[int(rng.integers(0, len(Q_BOUNDARY)))])
    k = int(K_POOL[int(rng.integers(0, len(K_POOL)))])
    b = int(B_POOL[int(rng.integers(0, len(B_POOL)))])
    fits = [L for L in L_POOL if k * b * L * q <= ELEMS_MAX and k * b * L * q * q <= WORK_MAX]
    L = int(fits[int(rng.integers(0, len(fits)))])           # (L = 1 always fits)
    if q <= 130 and b <= 4 and rng.random() < 0.35:
        L = int(L_LONG[int(rng.integers(0, 2))])
    zero = float(ZERO_FRACS[int(rng.integers(0, len(ZERO_FRACS)))])
    blank = bool(rng.random() < 0.3)                         # one position per sequence where nothing emits
    tiny = bool(rng.random() < 0.3)                          # a few entries at 1e-30 (below eps: clamped)
    eps = 1e-6 if rng.random() < 0.1 else 1e-16
    return dict(kind=kind, q=q, k=k, b=b, L=L, zero=zero, blank=blank, tiny=tiny, eps=eps)


def draw_model(rng, kind, q, m):
    """Model m of a case -> A (q,q) float32, rows summing to 1 (or to 0: the zeroed rows of "zero_absorb")."""
    if kind == "gene5":
        return gene_model(5, GENE_LENGTHS[m % len(GENE_LENGTHS)])
    if kind == "identity":
        return np.eye(q, dtype=np.float32)
    if kind == "cycle":                                      # a permutation matrix: shift by m + 1
        return np.roll(np.eye(q, dtype=np.float32), m + 1, axis=1)
    if kind == "ring":                                       # self + successor only
        A = np.eye(q) * (rng.random(q) * 0.8 + 0.1)[:, None]
        A[np.arange(q), (np.arange(q) + 1) % q] = 1.0 - A[np.arange(q), np.arange(q)]
        return A.astype(np.float32)
    A = rng.random((q, q)) ** 3 + 1e-3
    if kind == "sparse_diag":                                # as rand_model(dense=False), tests/test_engine_gpu.py
        A *= rng.random((q, q)) < 0.3
        A += np.eye(q) * 0.5
    elif kind == "block":
        A[: q // 2, q // 2:] = 0
        A[q // 2:, : q // 2] = 0
    elif kind == "zero_absorb":                              # as tests/stress_sweep.py kind 3: rows without successors
        rows = np.nonzero(rng.random(q) < 0.3)[0]
        A[rows] = 0
        absorbing = rows[rng.random(len(rows)) < 0.5]
        A[absorbing, absorbing] = 1.0
    A /= np.maximum(A.sum(-1, keepdims=True), 1e-30)
    return A.astype(np.float32)


def model_is_usable(A):
    """A draw the reference recursion has nothing to say about is rejected here, not skipped later: A must be finite,
    non-negative, every row summing to 1 or to 0, and not every row 0."""
    s = A.astype(np.float64).sum(-1)
    return bool(np.isfinite(A).all() and (A >= 0).all() and np.all((np.abs(s - 1) < 1e-4) | (s == 0)) and (s > 0).any())


def draw_case(rng):
    """-> dict(kind, q, k, b, L, zero, blank, tiny, eps, A (k,q,q), pi (k,q), E (k,b,L,q)) float32."""
    c = draw_shape(rng)
    k, b, L, q = c["k"], c["b"], c["L"], c["q"]
    As, pis = [], []
    for m in range(k):
        while True:
            A = draw_model(rng, c["kind"], q, m)
            if model_is_usable(A):
                break
        pi = rng.random(q) + 0.1
        As.append(A)
        pis.append((pi / pi.sum()).astype(np.float32))
    E = (rng.random((k, b, L, q)) * 0.9 + 0.05).astype(np.float32)
    if c["zero"] > 0:
        E[rng.random(E.shape) < c["zero"]] = 0.0
    if c["blank"]:
        t0 = rng.integers(0, L, size=(k, b))
        for m in range(k):
            E[m, np.arange(b), t0[m]] = 0.0
    if c["tiny"]:
        n = max(1, E.size // 1000)
        E.reshape(-1)[rng.integers(0, E.size, size=n)] = 1e-30
    c.update(A=np.stack(As), pi=np.stack(pis), E=E)
    return c


def make_case(A, pi, E, eps=1e-16, kind="given"):
    """A hand-made case in draw_case's format: A (k,q,q), pi (k,q), E (k,b,L,q)."""
    A, pi, E = np.asarray(A, np.float32), np.asarray(pi, np.float32), np.asarray(E, np.float32)
    k, b, L, q = E.shape
    return dict(kind=kind, q=q, k=k, b=b, L=L, zero=float((E == 0).mean()), blank=False, tiny=False, eps=eps,
                A=A.reshape(k, q, q), pi=pi.reshape(k, q), E=E)


# ---------------------------------------------------------------- the fp64 reference

def oracle(A, pi, E, eps):
    """One model: gamma64, ll64, log alpha64, log beta64 from ONE forward and ONE backward pass of oracle.textbook
    (the definitions of textbook.posterior / log_alpha / log_beta), plus U_t and Rb_t for the fp32-product emulation."""
    ah, cum = textbook.forward(A, pi, E, eps=eps)
    R, sc = textbook.backward(A, E, eps=eps)
    g = ah * R
    g /= g.sum(-1, keepdims=True)
    with np.errstate(divide="ignore"):
        la, lb = np.log(ah) + cum[..., None], np.log(R) + sc[..., None]
    return dict(g=g, ll=cum[:, -1], la=la, lb=lb, ah=ah, cum=cum, R=R)


def fp32_product_zeros(o):
    """CPU emulation of what k_lq_normalise reads: the parked product U_t * Rb_t (U_t = alpha_hat_t S_t, the
    unnormalised forward vector; fp64 recursion) rounded to fp32 -> (entries that are exactly 0, (sequence, t) rows
    with at least one).  Not a GPU measurement."""
    S = np.exp(np.diff(o["cum"], axis=1, prepend=0.0))
    with np.errstate(under="ignore"):
        prod = (o["ah"] * S[..., None] * o["R"]).astype(np.float32)
    z = prod == 0
    return int(z.sum()), int(z.any(-1).sum())


# ---------------------------------------------------------------- the checks

def _log_excess(x, x64):
    """assert_log_close_in_probability_space of tests/test_engine_gpu.py as a number: > 0 is a failure."""
    ref = x64.max(-1, keepdims=True)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        p, p64 = np.exp(np.minimum(x - ref, 50.0)), np.exp(x64 - ref)
        return float(np.nan_to_num(np.abs(p - p64) - (2e-5 + p64 * (3e-4 + 2e-7 * np.abs(ref))), nan=np.inf).max())


def _mx(a):
    return float(np.nan_to_num(a, nan=np.inf).max()) if a.size else 0.0


def engine_outputs(A, pi, E, eps):
    """Every output of the three entry points for A (k,q,q), pi (k,q), E (k,b,L,q) -> dict of numpy arrays."""
    import torch
    from hmm_layer_amd import engine
    t = lambda x: torch.as_tensor(np.asarray(x), dtype=torch.float32, device="cuda:0")
    Ad, pid, Ed = t(A), t(pi), t(E)
    out = {}
    for name, mode in (("prob", engine.POST_PROB), ("log", engine.POST_LOG), ("lognoll", engine.POST_LOG_NO_LL)):
        o, ll = engine.posterior(Ad, pid, Ed, mode=mode, eps=eps)
        out[name], out["ll_" + name] = o.cpu().numpy(), ll.cpu().numpy()
    la, ll = engine.forward(Ad, pid, Ed, eps=eps)
    out["la"], out["ll_fwd"] = la.cpu().numpy(), ll.cpu().numpy()
    _, ll = engine.forward(Ad, pid, Ed, want_log_alpha=False, eps=eps)
    out["ll_only"] = ll.cpu().numpy()
    out["lb"] = engine.backward(Ad, Ed, eps=eps).cpu().numpy()
    return out


def check_model(got, o, tag):
    """got: the outputs of ONE model (numpy, leading k axis removed); o: oracle() of it -> (failures, figures)."""
    fails, fig = [], {}
    g64, ll64 = o["g"], o["ll"]

    def need(ok, what, *val):
        if not ok:
            fails.append("%s: %s %s" % (tag, what, " ".join("%.3g" % v for v in val)))

    for name in ("prob", "log", "lognoll", "la", "lb"):
        need(not np.isnan(got[name]).any(), name + " has NaN")
        need(not (got[name] == np.inf).any(), name + " has +inf")
    for name in ("prob", "la", "lb"):
        need(np.isfinite(got[name]).all(), name + " is not entirely finite")
    fig["rowsum"] = _mx(np.abs(got["prob"].sum(-1) - 1))
    need(fig["rowsum"] <= 2e-5, "rows of POST_PROB do not sum to 1:", fig["rowsum"])
    fig["prob"] = _mx(np.abs(got["prob"] - g64))
    need(fig["prob"] <= 2e-5, "POST_PROB", fig["prob"])
    m = g64 > 1e-4
    lg64 = np.log(np.maximum(g64, 1e-300))
    for name, sub, tol in (("log", 0.0, 2e-5), ("lognoll", got["ll_lognoll"][:, None, None], 2e-5 + 2.4e-7 * np.abs(ll64).max())):
        with np.errstate(over="ignore", under="ignore", invalid="ignore"):
            lg = got[name] - sub
            fig[name] = _mx(np.abs(np.exp(lg) - g64))
            fig[name + "_logspace"] = _mx(np.abs(lg - lg64)[m])
        need(fig[name] <= tol, "exp(%s)" % name, fig[name], tol)
        need(fig[name + "_logspace"] <= 1e-3, "%s in log space" % name, fig[name + "_logspace"])
        fig[name + "_neginf"] = int((got[name] == -np.inf).sum())
    for name in ("la", "lb"):
        x, x64 = got[name], o[name]
        mm = x64 > -30
        with np.errstate(invalid="ignore"):
            fig[name] = _mx((np.abs(x - x64) - (3e-4 + 2e-7 * np.abs(x64)))[mm])
        need(fig[name] <= 0, "%s in log space, excess" % name, fig[name])
        fig[name + "_prob"] = _log_excess(x, x64)
        need(fig[name + "_prob"] <= 0, "%s in probability space, excess" % name, fig[name + "_prob"])
    for name in ("ll_prob", "ll_log", "ll_lognoll", "ll_fwd", "ll_only"):
        ex = _mx(np.abs(got[name] - ll64) - (1e-6 * np.abs(ll64) + 2e-4))
        fig["ll"] = max(fig.get("ll", -np.inf), ex)
        need(ex <= 0, name + " excess", ex)
        need(np.array_equal(got[name], got["ll_prob"]), name + " differs bitwise from the posterior's loglik")
    return fails, fig


def check_case(c, tag=""):
    """Runs the engine on the case and compares it with the oracle -> (failures, figures); figures["neginf"] is the
    number of -inf entries of the two log modes over all models."""
    k = c["k"]
    got = engine_outputs(c["A"], c["pi"], c["E"], c["eps"])
    fails, figs = [], {"neginf": 0}
    for m in range(k):
        o = oracle(c["A"][m], c["pi"][m], c["E"][m], c["eps"])
        f, fig = check_model({n: v[m] for n, v in got.items()}, o, "%s model %d" % (tag, m))
        fails += f
        figs["neginf"] += fig["log_neginf"] + fig["lognoll_neginf"]
        for n, v in fig.items():
            if not n.endswith("neginf"):
                figs[n] = max(figs.get(n, -np.inf), v)
        if k > 1:                                            # the models of a call do not interact: bitwise
            one = engine_outputs(c["A"][m:m + 1], c["pi"][m:m + 1], c["E"][m:m + 1], c["eps"])
            for n in got:
                if not np.array_equal(one[n][0], got[n][m], equal_nan=True):
                    d = one[n][0] != got[n][m]
                    fails.append("%s model %d: %s of the k = %d call differs from the k = 1 call in %d entries (first at %s)"
                                 % (tag, m, n, k, int(d.sum()), tuple(int(i) for i in np.argwhere(d)[0])))
    return fails, figs


def run(ncase, seed, verbose=True, first=0):
    """Cases first .. ncase-1 of `seed` -> number of failing cases (tests/test_largeq_sweep_gpu.py: must be 0)."""
    bad = 0
    for i in range(first, ncase):
        c = draw_case(case_rng(seed, i))
        fails, fig = check_case(c, "seed %d case %d" % (seed, i))
        bad += bool(fails)
        if verbose or fails:
            print("%s %3d %-11s q=%3d k=%d b=%3d L=%4d zero=%.2f%s%s eps=%.0e | post %.1e log %.1e/%.1e noll %.1e/%.1e rows %.1e"
                  " | la %+.1e %+.1e lb %+.1e %+.1e ll %+.1e | -inf %d" % (
                      "FAIL" if fails else "ok  ", i, c["kind"], c["q"], c["k"], c["b"], c["L"], c["zero"],
                      "b" if c["blank"] else " ", "t" if c["tiny"] else " ", c["eps"], fig["prob"], fig["log"],
                      fig["log_logspace"], fig["lognoll"], fig["lognoll_logspace"], fig["rowsum"], fig["la"],
                      fig["la_prob"], fig["lb"], fig["lb_prob"], fig["ll"], fig["neginf"]), flush=True)
        for f in fails[:12]:
            print("    " + f, flush=True)
    return bad


# ---------------------------------------------------------------- coverage of a (N, seed)

def coverage(shapes):
    """The coverage conditions as counts over a list of shapes -> dict (tests/test_largeq_sweep_cpu.py asserts them)."""
    qs = [s["q"] for s in shapes]
    return dict(
        boundary_missing=[q for q in Q_BOUNDARY if q not in qs],
        residues=sorted({q % 4 for q in qs}),
        slab_full=sum(q % 32 == 0 for q in qs), slab_tail=sum(q % 32 != 0 for q in qs),
        kinds={kd: sum(s["kind"] == kd for s in shapes) for kd in KINDS},
        zeros={z: sum(s["zero"] == z for s in shapes) for z in ZERO_FRACS},
        ragged_multi=sum(s["k"] >= 2 and s["b"] % 64 != 0 for s in shapes),
        lengths={L: sum(s["L"] == L for s in shapes) for L in L_POOL},
        long=sum(s["L"] in L_LONG for s in shapes),
        eps_large=sum(s["eps"] == 1e-6 for s in shapes),
        ks={k: sum(s["k"] == k for s in shapes) for k in K_POOL},
        bs={b: sum(s["b"] == b for s in shapes) for b in B_POOL})


def covered(cv):
    return (not cv["boundary_missing"] and cv["residues"] == [0, 1, 2, 3] and cv["slab_full"] >= 1 and cv["slab_tail"] >= 1
            and min(cv["kinds"].values()) >= 2 and min(cv["zeros"].values()) >= 2 and cv["ragged_multi"] >= 3
            and min(cv["lengths"].values()) >= 1 and cv["long"] >= 1 and cv["eps_large"] >= 1)


def search_seed(ncase, seeds=range(100000)):
    """The first seed whose first `ncase` shapes meet every coverage condition (how SEED was chosen for N_CASES)."""
    for seed in seeds:
        if covered(coverage([draw_shape(case_rng(seed, i)) for i in range(ncase)])):
            return seed
    return None


# ---------------------------------------------------------------- shared by the CPU and GPU test files

def lq_tile_width(b, q):
    """lq_tile_width of hmm_largeq.inc restated: the tile width (in 16-column units) with the cheapest critical path,
    (tiles per CU, rounded up) x width on 256 CUs; the first minimum wins."""
    mt = -(-b // 64)
    cost = {ntw: -(-(mt * -(-q // (16 * ntw))) // 256) * ntw for ntw in (4, 5, 6)}
    return min((4, 5, 6), key=lambda ntw: (cost[ntw], ntw))


def long_five_copy_case(L):
    """The five-copy gene model (71 states), b = 3, 47 % zeros iid (the emitter's zero fraction), random pi."""
    rng = np.random.default_rng(71000 + L)
    A = gene_model(5)
    pi = rng.random(71) + 0.1
    E = (rng.random((1, 3, L, 71)) * 0.9 + 0.05).astype(np.float32)
    E[rng.random(E.shape) < 0.47] = 0.0
    return make_case(A[None], (pi / pi.sum())[None], E, kind="gene5")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "search":
        print("seed:", search_seed(int(sys.argv[2]) if len(sys.argv) > 2 else N_CASES))
        sys.exit(0)
    nbad = run(int(sys.argv[1]) if len(sys.argv) > 1 else N_CASES, int(sys.argv[2]) if len(sys.argv) > 2 else SEED,
               first=int(sys.argv[3]) if len(sys.argv) > 3 else 0)
    print("failures:", nbad)
    sys.exit(1 if nbad else 0)
