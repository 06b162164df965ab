// hmm_scan_mid.inc — host side of the chunked scan for 17..64 states, included by hmm_engine.hip after the kernels
// (hmm_scan_rows.inc): one plan, one set of drivers.  The kernels are templates over the row width (NT tile rows);
// what else differs between the two widths — the model check and how the reduce stage is launched — lives in the
// traits types Scan32 / Scan64.

struct MidPlan {
    Plan p;                           // shape and chunking (k, b, L, q, NB, T, C, nchains; nsub = T / the width's SUB)
    long long nwaves;                 // apply waves: 16 (sequence, chunk) pairs each, never straddling models
    size_t o_ops, o_exps, o_prefix, o_llpre, o_suffix, o_lsuf, o_loglik, o_ckpt, o_phi, o_need, o_elig, o_nex;
    size_t o_risk, o_upi, total;      // the dense reduce's per-chain mark; hmm_backward's uniform start distribution
};

// W: the row width, Q32 or Q64.  T_fixed: a chunk length other than choose_T's (hmm_postgrad_chunked.inc).
static int make_midplan(int op, int k, int b, int L, int q, int W, MidPlan *pp, int T_fixed = 0) {
    if (k < 1 || b < 1 || L < 1 || q < 1) return HMM_ERR_BAD_SHAPE;
    if ((long long)k * b > (1ll << 30) / 64) return HMM_ERR_BAD_SHAPE;
    Plan &p = pp->p;
    p.k = k; p.b = b; p.L = L; p.q = q; p.NB = k * b;
    p.T = T_fixed ? T_fixed : choose_T(p.NB, L);
    p.C = (L + p.T - 1) / p.T;
    p.nsub = p.T / (W == Q32 ? Rows<2>::BLK : Rows<4>::BLK);
    p.nchains = (long long)p.NB * p.C;
    p.cpw = 16; p.seq_start = 1; p.G = 0; p.gsize = 0;
    pp->nwaves = (long long)k * (((long long)b * p.C + 15) / 16);
    size_t off = 0;
    pp->o_ops = off;    off = align_up(off + (size_t)p.nchains * W * W * sizeof(float));
    pp->o_exps = off;   off = align_up(off + (size_t)p.nchains * W * sizeof(int));
    pp->o_prefix = off; off = align_up(off + (size_t)p.nchains * W * sizeof(float));
    pp->o_llpre = off;  off = align_up(off + (size_t)p.nchains * sizeof(double));
    pp->o_suffix = off; off = align_up(off + (size_t)p.nchains * W * sizeof(float));
    pp->o_lsuf = off;   off = align_up(off + (size_t)p.nchains * sizeof(double));
    pp->o_loglik = off; off = align_up(off + (size_t)p.NB * sizeof(double));
    pp->o_phi = off;    off = align_up(off + (size_t)p.nchains * sizeof(float));
    pp->o_need = off;   off = align_up(off + (size_t)p.NB * sizeof(int));
    pp->o_elig = off;   off = align_up(off + (size_t)k * sizeof(int));
    pp->o_nex = off;    off = align_up(off + sizeof(int));
    pp->o_risk = off;   off = align_up(off + (size_t)p.nchains * sizeof(int));
    pp->o_upi = off;    off = align_up(off + (size_t)k * q * sizeof(float));
    pp->o_ckpt = off;
    if (op == HMM_OP_POSTERIOR)
        off = align_up(off + (size_t)pp->nwaves * p.nsub * 16 * W * sizeof(float));
    pp->total = off;
    return HMM_OK;
}

// the row width serving (k, b, L, q): Q32 for 17..32 states, Q64 for few long sequences of 33..64, 0 = no chunked scan
static int mid_width(int k, int b, int L, int q) {
    if (q > QP && q <= Q32) return Q32;
    return scan64_wanted(k, b, L, q) ? Q64 : 0;
}

// the regions of the chunked scan's workspace (MidPlan::o_*), typed
struct WsMid {
    float *ops; int *exps; float *prefix; double *llpre; float *suffix; double *lsuf, *loglik; float *ckpt, *phi;
    int *need, *elig, *nex, *risk; float *upi;
#define WSMID(m) m(ws_at<std::remove_pointer_t<decltype(m)>>(ws, pp.o_##m))
    WsMid(const MidPlan &pp, const void *ws)
        : WSMID(ops), WSMID(exps), WSMID(prefix), WSMID(llpre), WSMID(suffix), WSMID(lsuf), WSMID(loglik), WSMID(ckpt),
          WSMID(phi), WSMID(need), WSMID(elig), WSMID(nex), WSMID(risk), WSMID(upi) {}
#undef WSMID
};

// ---- what differs between the widths on the host: how the model check and the reduce stage are launched
struct Scan32 {
    static constexpr int NT = 2, W = Rows<NT>::W;
    // exact_mode: the routing mode the verdict is formed under (default: the option's); elig: where it goes (default:
    // the plan's elig[k]).  The sequence-sharded calls ask twice: HMM_EXACT_OFF for the scan, HMM_EXACT_AUTO for the
    // model's primitivity.
    static void check(const float *A, const MidPlan &pp, float eps, char *ws, hipStream_t st, int exact_mode = -1,
                      int *elig = nullptr) {
        const WsMid w(pp, ws);
        launch(k32_check, dim3(pp.p.k), dim3(64), 0, st, A, elig ? elig : w.elig, pp.p.q,
               exact_mode < 0 ? opt(HMM_OPT_EXACT) : exact_mode, eps, w.nex, opt(HMM_OPT_FORCE_DENSE) == 1 ? 1 : 0);
    }
    // the compiled sparse topology first, then the dense reduce for the models outside it
    static void reduce(const float *A, const float *E, const MidPlan &pp, float eps, char *ws, hipStream_t st) {
        const Plan &p = pp.p;
        const WsMid w(pp, ws);
        const unsigned nb = (unsigned)((p.nchains + 4 * RsCfg<TopoGene29>::CPW - 1) / (4 * RsCfg<TopoGene29>::CPW));
        launch(k_reduce_sparse_wide<TopoGene29>, dim3(nb), dim3(256), 0, st, A, E, w.ops, w.exps, w.elig, p, eps);
        if (p.k > 1 || !HMM_RS_UNI)                // waves that straddle two models
            launch(k_reduce_sparse_wide<TopoGene29, true>, dim3(nb), dim3(256), 0, st, A, E, w.ops, w.exps, w.elig, p, eps);
        // every chain its own wave (grid stride; exits at once for the models the sparse kernels served)
        const long long nbd = (p.nchains + 3) / 4;
        launch(reduce_dense<NT>, dim3((unsigned)(nbd < 8192 ? nbd : 8192)), dim3(256), 0, st, A, E, w.ops, w.exps, w.risk,
               w.elig, p, eps);
    }
};

struct Scan64 {
    static constexpr int NT = 4, W = Rows<NT>::W;
    // (exact_mode given — the sequence-sharded calls —: nseq = 0 keeps the sparse models' routing rule out of it)
    static void check(const float *A, const MidPlan &pp, float eps, char *ws, hipStream_t st, int exact_mode = -1,
                      int *elig = nullptr) {
        const WsMid w(pp, ws);
        launch(k64_check, dim3(pp.p.k), dim3(64), 0, st, A, elig ? elig : w.elig, pp.p.q,
               exact_mode < 0 ? opt(HMM_OPT_EXACT) : exact_mode, eps, w.nex, exact_mode < 0 ? pp.p.NB : 0,
               opt(HMM_OPT_FORCE_DENSE) == 1 ? 1 : 0);
    }
    static void reduce(const float *A, const float *E, const MidPlan &pp, float eps, char *ws, hipStream_t st) {
        const Plan &p = pp.p;
        const WsMid w(pp, ws);
        const long long nbd = (p.nchains + 3) / 4;
        launch(reduce_dense<NT>, dim3((unsigned)(nbd < 8192 ? nbd : 8192)), dim3(256), 0, st, A, E, w.ops, w.exps, w.risk,
               w.elig, p, eps);
    }
};

// ---- the drivers, S = Scan32 or Scan64

static dim3 mid_grid(const MidPlan &pp) { return dim3((unsigned)((pp.nwaves + 3) / 4)); }

template <class S>
static void scan_reduce_scan(const float *A, const float *pi, const float *E, const MidPlan &pp, float eps, char *ws,
                             hipStream_t st) {
    const WsMid w(pp, ws);
    S::check(A, pp, eps, ws, st);
    S::reduce(A, E, pp, eps, ws, st);
    launch(scan<S::NT>, dim3(pp.p.NB), dim3(128), 0, st, pi, w.ops, w.exps, w.prefix, w.llpre, w.suffix, w.lsuf, w.loglik,
           w.elig, pp.p, eps, nullptr, nullptr, nullptr, nullptr);
}

// need[] from the certificate sums phi (or null: the reduces' marks only); one kernel for both widths
template <class S>
static void scan_select(const MidPlan &pp, const WsMid &w, const float *phi, hipStream_t st) {
    launch(k_scan_select, dim3((pp.p.NB + 255) / 256), dim3(256), 0, st, w.elig, phi, w.need, w.nex, pp.p, 0.f,
           opt(HMM_OPT_EXACT), w.exps, w.risk, S::W);
}

// log-likelihoods of the models the chunked path serves -> ws loglik; need[] for the others.  The log-likelihood comes
// out of the chunk scan; the forward apply kernel runs for the certificate only (forward<false, true>), as
// hmm_forward's scan plan does for 16 states.
template <class S>
static void scan_loglik(const float *A, const float *pi, const float *E, const MidPlan &pp, float eps, char *ws,
                        hipStream_t st) {
    const WsMid w(pp, ws);
    scan_reduce_scan<S>(A, pi, E, pp, eps, ws, st);
    const bool cert = opt(HMM_OPT_EXACT) == HMM_EXACT_AUTO;
    if (cert)
        launch(forward<S::NT, false, true>, mid_grid(pp), dim3(256), 0, st, A, E, w.prefix, nullptr, nullptr, nullptr,
               w.elig, pp.p, eps, pp.nwaves, w.suffix, w.phi);
    scan_select<S>(pp, w, cert ? w.phi : nullptr, st);
}

template <class S>
static void scan_posterior(const float *A, const float *pi, const float *E, const MidPlan &pp, float eps, int mode,
                           float *out, char *ws, hipStream_t st, const DecodeMid *dec) {
    const WsMid w(pp, ws);
    scan_reduce_scan<S>(A, pi, E, pp, eps, ws, st);
    launch(forward<S::NT, false, false>, mid_grid(pp), dim3(256), 0, st, A, E, w.prefix, nullptr, w.ckpt, nullptr, w.elig,
           pp.p, eps, pp.nwaves, nullptr, nullptr);
    if (dec) {                                               // hmm_posterior_decode_mid (HMM_POST_PROB, no `out`)
        launch(backward<S::NT, 0, false, DecodeMid>, mid_grid(pp), dim3(256), 0, st, A, E, w.ckpt, w.suffix, nullptr,
               nullptr, nullptr, w.phi, w.elig, pp.p, eps, pp.nwaves, nullptr, *dec);
        scan_select<S>(pp, w, w.phi, st);
        return;
    }
    auto *kern = mode == HMM_POST_PROB ? backward<S::NT, 0, false>
                 : mode == HMM_POST_LOG ? backward<S::NT, 1, false> : backward<S::NT, 2, false>;
    launch(kern, mid_grid(pp), dim3(256), 0, st, A, E, w.ckpt, w.suffix, w.lsuf, w.loglik, out, w.phi, w.elig, pp.p, eps,
           pp.nwaves, nullptr, NoDecode());
    scan_select<S>(pp, w, w.phi, st);
}

// log alpha (and the log-likelihoods) of the models the chunked path serves; need[] for the others.  The certificate
// variant runs whatever the routing mode, so that EXACT_OFF and the automatic routing compute an unflagged sequence
// with the same kernel.
template <class S>
static void scan_forward(const float *A, const float *pi, const float *E, const MidPlan &pp, float eps, float *log_alpha,
                         char *ws, hipStream_t st) {
    const WsMid w(pp, ws);
    scan_reduce_scan<S>(A, pi, E, pp, eps, ws, st);
    launch(forward<S::NT, true, true>, mid_grid(pp), dim3(256), 0, st, A, E, w.prefix, w.llpre, nullptr, log_alpha, w.elig,
           pp.p, eps, pp.nwaves, w.suffix, w.phi);
    scan_select<S>(pp, w, w.phi, st);
}

// log beta of the models the chunked path serves; need[] for the others.  hmm_backward has no start distribution: the
// chunk scan's forward half, whose vectors weigh the certificate (the backward kernel's CERT3), starts from the
// uniform one.
template <class S>
static void scan_backward(const float *A, const float *E, const MidPlan &pp, float eps, float *log_beta, char *ws,
                          hipStream_t st) {
    const WsMid w(pp, ws);
    (void)hipMemsetD32Async((hipDeviceptr_t)w.upi, __builtin_bit_cast(int, 1.0f / (float)pp.p.q), (size_t)pp.p.k * pp.p.q,
                            st);
    scan_reduce_scan<S>(A, w.upi, E, pp, eps, ws, st);
    launch(backward<S::NT, 3, true>, mid_grid(pp), dim3(256), 0, st, A, E, nullptr, w.suffix, w.lsuf, nullptr, log_beta,
           w.phi, w.elig, pp.p, eps, pp.nwaves, w.prefix, NoDecode());
    scan_select<S>(pp, w, w.phi, st);
}
