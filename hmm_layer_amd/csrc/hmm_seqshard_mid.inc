// Sequence-sharded forward-backward for 17..64 states: hmm_seqshard.inc's protocol on the chunked scan of
// hmm_scan_rows.inc / hmm_scan_mid.inc (included after hmm_scan_mid.inc), with W x W operators, W = QT = 32 (17..32
// states) or 64.
//
// Every rank owns one contiguous time slab of EVERY sequence, E_slab (k, b, Ls, q):
//
//   1. hmm_seqshard_mid_reduce     local: the slab's chunk operators (S::reduce: the compiled sparse reduce or
//                                  reduce_dense<NT>), composed into ONE operator per sequence (compose<NT>: groups of
//                                  ~sqrt(C) chunks first when the slab has SCAN2_MIN_C chunks or more, then the groups):
//                                  (k,b,QT,QT) fp32 + (k,b,QT) int32 column exponents
//   2. all-gather                  the host lays the ranks' operators out (k,b,R,...)
//   3. hmm_seqshard_mid_posterior  local: scan<NT>'s hops over the R slab operators of every sequence leave the vectors
//                                  entering every slab and the total log-likelihood; the vectors entering THIS slab
//                                  start the scan over its own chunk operators (still in the workspace), then
//                                  forward<NT> / backward<NT> as in hmm_posterior
//
// A slab that does not begin at position 0 has Plan::seq_start = 0: its first position takes a transition like any
// other (reduce_dense, reduce_sparse_wave, make_chain_tile).  The serial kernels of hmm_midq.inc cannot be cut in time,
// so these calls run the scan for every model (the model check under HMM_EXACT_OFF) and hand the host what it needs to
// decide: phi_out, the slab's share of psi plus a whole 1 per chain a reduce marked, +inf for a model whose support is
// not primitive (the same check under HMM_EXACT_AUTO, into a second verdict per model).  The local scan walks the
// slab's C chunks in one level.

struct SsMidPlan {
    MidPlan mp;
    int W, G, gsize;         // row width; two-level compose: G groups of gsize chunks per sequence (G = 0: one level)
    size_t o_gops, o_gexps;  // the group operators [NB][G][W][W], [NB][G][W]
    size_t o_gsc_pre, o_gsc_ll, o_gsc_suf, o_gsc_ls, o_gsc_total;   // the global hops' vectors [NB][R][W], [NB][R]; [NB]
    size_t o_entry_pre, o_entry_ll, o_entry_suf, o_entry_ls;        // ... those entering this slab [NB][W], [NB]
    size_t o_elig2;          // the model check under HMM_EXACT_AUTO [k]: 0 = support not primitive
    size_t total;
};

static int ssm_tile(int q) { return q > QP && q <= Q32 ? Q32 : (q > Q32 && q <= Q64 ? Q64 : 0); }

static int make_ssmidplan(int k, int b, int Ls, int q, int R, SsMidPlan *sp) {
    sp->W = ssm_tile(q);
    if (!sp->W) return HMM_ERR_Q_UNSUPPORTED;
    if (R < 1) return HMM_ERR_BAD_ARGUMENT;
    const int rc = make_midplan(HMM_OP_POSTERIOR, k, b, Ls, q, sp->W, &sp->mp);
    if (rc) return rc;
    const Plan &p = sp->mp.p;
    const size_t W = (size_t)sp->W;
    sp->G = 0; sp->gsize = 0;
    if (p.C >= SCAN2_MIN_C) {
        int gs = 1;
        while (gs * gs < p.C) ++gs;
        sp->gsize = gs;
        sp->G = (p.C + gs - 1) / gs;
    }
    size_t off = sp->mp.total;
    const size_t ng = (size_t)p.NB * (sp->G > 0 ? sp->G : 1), nr = (size_t)p.NB * R;
    sp->o_gops = off;      off = align_up(off + ng * W * W * sizeof(float));
    sp->o_gexps = off;     off = align_up(off + ng * W * sizeof(int));
    sp->o_gsc_pre = off;   off = align_up(off + nr * W * sizeof(float));
    sp->o_gsc_ll = off;    off = align_up(off + nr * sizeof(double));
    sp->o_gsc_suf = off;   off = align_up(off + nr * W * sizeof(float));
    sp->o_gsc_ls = off;    off = align_up(off + nr * sizeof(double));
    sp->o_gsc_total = off; off = align_up(off + (size_t)p.NB * sizeof(double));
    sp->o_entry_pre = off; off = align_up(off + (size_t)p.NB * W * sizeof(float));
    sp->o_entry_ll = off;  off = align_up(off + (size_t)p.NB * sizeof(double));
    sp->o_entry_suf = off; off = align_up(off + (size_t)p.NB * W * sizeof(float));
    sp->o_entry_ls = off;  off = align_up(off + (size_t)p.NB * sizeof(double));
    sp->o_elig2 = off;     off = align_up(off + (size_t)p.k * sizeof(int));
    sp->total = off;
    return HMM_OK;
}

template <class S>
static void ssm_reduce(const float *A, const float *E, const SsMidPlan &sp, float eps, char *ws, float *slab_op,
                       int *slab_exp, hipStream_t st) {
    const MidPlan &pp = sp.mp;
    const Plan &p = pp.p;
    const WsMid w(pp, ws);
    S::check(A, pp, eps, ws, st, HMM_EXACT_AUTO, ws_at<int>(ws, sp.o_elig2));   // primitivity, for phi_out
    S::check(A, pp, eps, ws, st, HMM_EXACT_OFF);                                // the scan serves every model here
    S::reduce(A, E, pp, eps, ws, st);
    // all chunk operators of a sequence -> one: groups first, then the groups
    const float *ops = w.ops;
    const int *exps = w.exps;
    Plan pc = p;
    if (sp.G > 0) {
        pc.G = sp.G; pc.gsize = sp.gsize;
        const long long nwv = (long long)p.NB * sp.G;
        launch(compose<S::NT>, dim3((unsigned)((nwv + 3) / 4)), dim3(256), 0, st, ops, exps, ws_at<float>(ws, sp.o_gops),
               ws_at<int>(ws, sp.o_gexps), pc);
        ops = ws_at<float>(ws, sp.o_gops);
        exps = ws_at<int>(ws, sp.o_gexps);
        pc.C = sp.G;
    }
    pc.G = 1;
    pc.gsize = pc.C;
    launch(compose<S::NT>, dim3((unsigned)((p.NB + 3) / 4)), dim3(256), 0, st, ops, exps, slab_op, slab_exp, pc);
}

template <class S>
static void ssm_posterior(const float *A, const float *pi, const float *E, const SsMidPlan &sp, float eps,
                          const float *all_ops, const int *all_exps, int R, int r, int mode, float *out, double *loglik,
                          float *phi_out, char *ws, hipStream_t st) {
    const MidPlan &pp = sp.mp;
    const Plan &p = pp.p;
    const WsMid w(pp, ws);
    constexpr int W = S::W;
    // the hops over the R slab operators of every sequence (layout [seq][slab]): the vectors entering every slab and
    // the total log-likelihood
    Plan pg = p;
    pg.C = R;
    pg.seq_start = 1;
    float *gpre = ws_at<float>(ws, sp.o_gsc_pre), *gsuf = ws_at<float>(ws, sp.o_gsc_suf);
    double *gll = ws_at<double>(ws, sp.o_gsc_ll), *gls = ws_at<double>(ws, sp.o_gsc_ls);
    double *total = ws_at<double>(ws, sp.o_gsc_total);
    launch(scan<S::NT>, dim3(p.NB), dim3(128), 0, st, pi, all_ops, all_exps, gpre, gll, gsuf, gls, total, w.elig, pg, eps,
           nullptr, nullptr, nullptr, nullptr);
    float *epre = ws_at<float>(ws, sp.o_entry_pre), *esuf = ws_at<float>(ws, sp.o_entry_suf);
    double *ell = ws_at<double>(ws, sp.o_entry_ll), *els = ws_at<double>(ws, sp.o_entry_ls);
    launch(k_mid_pick, dim3((unsigned)(((long long)p.NB * W + 255) / 256)), dim3(256), 0, st, gpre, gll, gsuf, gls, epre,
           ell, esuf, els, p.NB, R, r, W);
    // the local chunk scan from those vectors (the slab's chunk operators are still in the workspace)
    launch(scan<S::NT>, dim3(p.NB), dim3(128), 0, st, pi, w.ops, w.exps, w.prefix, w.llpre, w.suffix, w.lsuf, w.loglik,
           w.elig, p, eps, r == 0 ? nullptr : epre, r == 0 ? nullptr : ell, esuf, els);
    // the sequence's log-likelihood is the global hops', not the local prefix's
    launch(k_copy_loglik, dim3((p.NB + 255) / 256), dim3(256), 0, st, total, w.loglik, p.NB);
    launch(forward<S::NT, false, false>, mid_grid(pp), dim3(256), 0, st, A, E, w.prefix, nullptr, w.ckpt, nullptr, w.elig, p,
           eps, pp.nwaves, nullptr, nullptr);
    auto *kern = mode == HMM_POST_PROB ? backward<S::NT, 0, false>
                 : mode == HMM_POST_LOG ? backward<S::NT, 1, false> : backward<S::NT, 2, false>;
    launch(kern, mid_grid(pp), dim3(256), 0, st, A, E, w.ckpt, w.suffix, w.lsuf, w.loglik, out, w.phi, w.elig, p, eps,
           pp.nwaves, nullptr, NoDecode());
    if (loglik) launch(k_copy_loglik, dim3((p.NB + 255) / 256), dim3(256), 0, st, total, loglik, p.NB);
    if (phi_out)
        launch(k_mid_phi, dim3((p.NB + 255) / 256), dim3(256), 0, st, w.phi, w.elig, ws_at<int>(ws, sp.o_elig2), w.exps,
               w.risk, phi_out, p, W);
}

extern "C" {

int hmm_seqshard_mid_max_states(void) { return Q64; }

int hmm_seqshard_mid_tile(int q) { return ssm_tile(q); }

size_t hmm_seqshard_mid_workspace_bytes(int k, int b, int Ls, int q, int R) {
    SsMidPlan sp;
    if (make_ssmidplan(k, b, Ls, q, R, &sp)) return 0;
    return sp.total;
}

int hmm_seqshard_mid_reduce(const float *A, const float *E, int k, int b, int Ls, int q, float eps, int seq_start, int R,
                            float *slab_op, int *slab_exp, void *workspace, size_t workspace_bytes, void *stream) {
    SsMidPlan sp;
    const int rc = make_ssmidplan(k, b, Ls, q, R, &sp);
    if (rc) return rc;
    if (!A || !E || !slab_op || !slab_exp || !workspace) return HMM_ERR_NULL_POINTER;
    if (check_eps(eps)) return HMM_ERR_BAD_ARGUMENT;
    if (workspace_bytes < sp.total || ((uintptr_t)workspace & 255)) return HMM_ERR_WORKSPACE;
    sp.mp.p.seq_start = seq_start ? 1 : 0;
    if (sp.W == Q32) ssm_reduce<Scan32>(A, E, sp, eps, (char *)workspace, slab_op, slab_exp, (hipStream_t)stream);
    else ssm_reduce<Scan64>(A, E, sp, eps, (char *)workspace, slab_op, slab_exp, (hipStream_t)stream);
    return check_launch();
}

int hmm_seqshard_mid_posterior(const float *A, const float *pi, const float *E, int k, int b, int Ls, int q, float eps,
                               int seq_start, const float *all_ops, const int *all_exps, int R, int r, int mode,
                               float *out, double *loglik, float *phi_out, void *workspace, size_t workspace_bytes,
                               void *stream) {
    SsMidPlan sp;
    const int rc = make_ssmidplan(k, b, Ls, q, R, &sp);
    if (rc) return rc;
    if (r < 0 || r >= R || (seq_start != 0) != (r == 0)) return HMM_ERR_BAD_ARGUMENT;
    if (mode < HMM_POST_PROB || mode > HMM_POST_LOG_NO_LL) return HMM_ERR_BAD_ARGUMENT;
    if (!A || !pi || !E || !all_ops || !all_exps || !out || !workspace) return HMM_ERR_NULL_POINTER;
    if (check_eps(eps)) return HMM_ERR_BAD_ARGUMENT;
    if (workspace_bytes < sp.total || ((uintptr_t)workspace & 255)) return HMM_ERR_WORKSPACE;
    sp.mp.p.seq_start = seq_start ? 1 : 0;
    if (sp.W == Q32)
        ssm_posterior<Scan32>(A, pi, E, sp, eps, all_ops, all_exps, R, r, mode, out, loglik, phi_out, (char *)workspace,
                              (hipStream_t)stream);
    else
        ssm_posterior<Scan64>(A, pi, E, sp, eps, all_ops, all_exps, R, r, mode, out, loglik, phi_out, (char *)workspace,
                              (hipStream_t)stream);
    return check_launch();
}

}  // extern "C"
