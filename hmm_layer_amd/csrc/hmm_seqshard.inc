// Sequence-sharded forward-backward: the chunk scan lifted across devices (included by hmm_engine.hip).
//
// SURVEY.md 8(f) rank 4.  For few very long sequences the batch cannot be cut across GPUs; time can.
// Each rank owns one contiguous time slab of EVERY sequence, E_slab (k, b, Ls, q), and the roles of
// TotalProbabilityCell.forward (hmm_layer/TotalProbabilityCell.py:30-49) and
// _get_total_forward_from_chunks / _get_total_backward_from_chunks (hmm_layer/MsaHMMLayer.py:285-319,
// 384-419) — stitching conditional chunk results into totals — are played once more, one level up:
//
//   1. hmm_seqshard_reduce      local: chunk operators of the slab (the reduce kernels), composed into
//                               ONE operator per sequence (k_scan_compose, twice): (k,b,16,16) fp32 +
//                               (k,b,16) int32 exponents = 1.1 KB per sequence
//   2. all-gather               the host exchanges the slab operators (RCCL all-gather over xGMI; the
//                               only collective of this mode) and lays them out (k,b,R,...)
//   3. hmm_seqshard_posterior   local: the chunk scan's hops (k_scan) over the R slab operators — every
//                               rank repeats these few hops and reads off the vectors ENTERING ITS OWN
//                               slab (alpha_hat from the slabs before, beta from the slabs after) and
//                               the total log-likelihood — then the usual scan over its own chunk
//                               operators started from those vectors, and the apply kernels.
//
// Nothing else changes: the operators of step 1 are kept in the workspace for step 3, the in-chunk
// arithmetic is the apply kernels' exact cell step, and a slab that does not begin at position 0
// simply has no "first observation" (Plan::seq_start = 0).  The serial exact-clamp kernels cannot be
// sharded in time; instead every rank returns each sequence's local floor-transition bound (the
// certificate of k_backward, see there; +inf for models whose support is not primitive), the host sums
// it over ranks and, above 1e-6, gathers that sequence on one device for the unsharded call.

// phi_out[seq] = the slab's share of the sequence's clamp-born posterior mass (psi of backward_body,
// summed over the slab's chunks); +inf when the model is not primitive
// (a chunk whose operator columns went through the denormal range counts as flagged: reduce_sparse_wave's mark in the
// pad lane of the exponent row, see k_exact_select)
__global__ __launch_bounds__(256) void k_seqshard_phi(const float *__restrict__ psi, const int *__restrict__ topo_auto,
                                                      float *__restrict__ phi_out, Plan p, float eps,
                                                      const int *__restrict__ exps) {
    const int seq = blockIdx.x * 256 + threadIdx.x;
    if (seq >= p.NB) return;
    const int tpv = topo_auto[seq / p.b];
    float s = 0.f;
    for (int c = 0; c < p.C; ++c) {
        s += psi[(size_t)seq * p.C + c];
        if (exps && tpv != 0 && exps[((size_t)seq * p.C + c) * QP + QP - 1] != 0) s += 1.f;
    }
    phi_out[seq] = tpv == TOPO_EXACT ? __builtin_inff() : s;
}

struct SsPlan {
    Plan p;
    size_t o_gsc_pre, o_gsc_ll, o_gsc_suf, o_gsc_ls, o_gsc_total, o_entry_pre, o_entry_ll, o_entry_suf, o_entry_ls,
        o_topo2, o_c2ops, o_c2exps, total;
};

static int make_ssplan(int k, int b, int Ls, int q, int R, SsPlan *sp) {
    if (R < 1) return HMM_ERR_BAD_ARGUMENT;
    int rc = make_plan(HMM_OP_POSTERIOR, k, b, Ls, q, &sp->p);
    if (rc) return rc;
    const Plan &p = sp->p;
    size_t off = p.total;
    const size_t nr = (size_t)p.NB * R;
    sp->o_gsc_pre = off;   off = align_up(off + nr * QP * sizeof(float));
    sp->o_gsc_ll = off;    off = align_up(off + nr * sizeof(double));
    sp->o_gsc_suf = off;   off = align_up(off + nr * QP * sizeof(float));
    sp->o_gsc_ls = off;    off = align_up(off + nr * sizeof(double));
    sp->o_gsc_total = off; off = align_up(off + (size_t)p.NB * sizeof(double));
    sp->o_entry_pre = off; off = align_up(off + (size_t)p.NB * QP * sizeof(float));
    sp->o_entry_ll = off;  off = align_up(off + (size_t)p.NB * sizeof(double));
    sp->o_entry_suf = off; off = align_up(off + (size_t)p.NB * QP * sizeof(float));
    sp->o_entry_ls = off;  off = align_up(off + (size_t)p.NB * sizeof(double));
    sp->o_topo2 = off;     off = align_up(off + (size_t)p.k * 2 * sizeof(int));
    sp->o_c2ops = off;     off = align_up(off + (size_t)p.NB * QP * QP * sizeof(float));
    sp->o_c2exps = off;    off = align_up(off + (size_t)p.NB * QP * sizeof(int));
    sp->total = off;
    return HMM_OK;
}

// entry vectors of slab r out of the global scan's per-slab vectors [seq][R]
__global__ __launch_bounds__(256) void k_seqshard_pick(const float *__restrict__ gpre, const double *__restrict__ gll,
                                                       const float *__restrict__ gsuf, const double *__restrict__ gls,
                                                       float *__restrict__ pre, double *__restrict__ ll,
                                                       float *__restrict__ suf, double *__restrict__ ls, int NB, int R,
                                                       int r) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= NB * QP) return;
    const int seq = i / QP, n = i - seq * QP;
    pre[i] = gpre[((size_t)seq * R + r) * QP + n];
    suf[i] = gsuf[((size_t)seq * R + r) * QP + n];
    if (n == 0) { ll[seq] = gll[(size_t)seq * R + r]; ls[seq] = gls[(size_t)seq * R + r]; }
}

extern "C" {

size_t hmm_seqshard_workspace_bytes(int k, int b, int Ls, int q, int R) {
    SsPlan sp;
    if (q > QP || make_ssplan(k, b, Ls, q, R, &sp)) return 0;
    return sp.total;
}

int hmm_seqshard_reduce(const float *A, const float *E, int k, int b, int Ls, int q, float eps, int seq_start,
                        int R, float *slab_op, int *slab_exp, void *workspace, size_t workspace_bytes, void *stream) {
    if (q > QP) return HMM_ERR_Q_UNSUPPORTED;
    SsPlan sp;
    int rc = make_ssplan(k, b, Ls, q, R, &sp);
    if (rc) return rc;
    if (!A || !E || !slab_op || !slab_exp || !workspace) return HMM_ERR_NULL_POINTER;
    if (check_eps(eps)) return HMM_ERR_BAD_ARGUMENT;
    if (workspace_bytes < sp.total || ((uintptr_t)workspace & 255)) return HMM_ERR_WORKSPACE;
    Plan p = sp.p;
    p.seq_start = seq_start ? 1 : 0;
    char *ws = (char *)workspace;
    hipStream_t st = (hipStream_t)stream;
    int *topo2 = (int *)(ws + sp.o_topo2);
    // the model's primitivity, for the certificate the host collects (the scan serves every model here)
    hipLaunchKernelGGL(k_topo_check, dim3(p.k), dim3(64), 0, st, A, topo2, p.k, p.q, 0, HMM_EXACT_AUTO, eps, topo2 + p.k);
    run_reduce(A, E, p, eps, ws, st, nullptr, HMM_EXACT_OFF);
    // all chunk operators of a sequence -> one: groups first, then the groups
    const float *ops = (const float *)(ws + p.o_ops);
    const int *exps = (const int *)(ws + p.o_exps);
    const int *topo = (const int *)(ws + p.o_topo);
    Plan pc = p;
    if (p.G > 0) {
        const long long nwv = (long long)p.NB * p.G;
        hipLaunchKernelGGL(k_scan_compose, dim3((unsigned)((nwv + 3) / 4)), dim3(256), 0, st, ops, exps,
                           (float *)(ws + p.o_gops), (int *)(ws + p.o_gexps), topo, p);
        ops = (const float *)(ws + p.o_gops);
        exps = (const int *)(ws + p.o_gexps);
        pc.C = p.G;
    }
    pc.G = 1;
    pc.gsize = pc.C;
    hipLaunchKernelGGL(k_scan_compose, dim3((unsigned)((p.NB + 3) / 4)), dim3(256), 0, st, ops, exps, slab_op, slab_exp,
                       topo, pc);
    return check_launch();
}

int hmm_seqshard_posterior(const float *A, const float *pi, const float *E, int k, int b, int Ls, int q, float eps,
                           int seq_start, const float *all_ops, const int *all_exps, int R, int r, int mode,
                           float *out, double *loglik, float *phi_out, void *workspace, size_t workspace_bytes,
                           void *stream) {
    if (q > QP) return HMM_ERR_Q_UNSUPPORTED;
    SsPlan sp;
    int rc = make_ssplan(k, b, Ls, q, R, &sp);
    if (rc) return rc;
    if (r < 0 || r >= R || (seq_start != 0) != (r == 0)) return HMM_ERR_BAD_ARGUMENT;
    if (mode < HMM_POST_PROB || mode > HMM_POST_LOG_NO_LL) return HMM_ERR_BAD_ARGUMENT;
    if (!A || !pi || !E || !all_ops || !all_exps || !out || !workspace) return HMM_ERR_NULL_POINTER;
    if (check_eps(eps)) return HMM_ERR_BAD_ARGUMENT;
    if (workspace_bytes < sp.total || ((uintptr_t)workspace & 255)) return HMM_ERR_WORKSPACE;
    Plan p = sp.p;
    p.seq_start = seq_start ? 1 : 0;
    char *ws = (char *)workspace;
    hipStream_t st = (hipStream_t)stream;
    const int *topo = (const int *)(ws + p.o_topo);
    // the chunk scan's hops over the R slab operators of every sequence (layout [seq][slab]): vectors
    // entering every slab and the total log-likelihood
    Plan pg = p;
    pg.C = R;
    pg.seq_start = 1;
    float *gpre = (float *)(ws + sp.o_gsc_pre), *gsuf = (float *)(ws + sp.o_gsc_suf);
    double *gll = (double *)(ws + sp.o_gsc_ll), *gls = (double *)(ws + sp.o_gsc_ls);
    double *total = (double *)(ws + sp.o_gsc_total);
    hipLaunchKernelGGL(k_scan, dim3(p.NB), dim3(128), 0, st, pi, all_ops, all_exps, gpre, gll, gsuf, gls, total, topo, pg,
                       eps);
    float *epre = (float *)(ws + sp.o_entry_pre), *esuf = (float *)(ws + sp.o_entry_suf);
    double *ell = (double *)(ws + sp.o_entry_ll), *els = (double *)(ws + sp.o_entry_ls);
    hipLaunchKernelGGL(k_seqshard_pick, dim3((p.NB * QP + 255) / 256), dim3(256), 0, st, (const float *)gpre,
                       (const double *)gll, (const float *)gsuf, (const double *)gls, epre, ell, esuf, els, p.NB, R, r);
    // the local chunk scan from those vectors (the slab's chunk operators are still in the workspace)
    run_scan(pi, p, eps, ws, st, nullptr, r == 0 ? nullptr : (const float *)epre, r == 0 ? nullptr : (const double *)ell,
             (const float *)esuf, (const double *)els);
    // the sequence's log-likelihood is the global scan's, not the local prefix's
    hipLaunchKernelGGL(k_copy_loglik, dim3((p.NB + 255) / 256), dim3(256), 0, st, (const double *)total,
                       (double *)(ws + p.o_loglik), p.NB);
    if ((rc = s16_apply(A, pi, E, p, eps, mode, ws, out, loglik, st, nullptr, false))) return rc;
    if (phi_out)
        hipLaunchKernelGGL(k_seqshard_phi, dim3((p.NB + 255) / 256), dim3(256), 0, st, (const float *)(ws + p.o_phi),
                           (const int *)(ws + sp.o_topo2), phi_out, p, eps, (const int *)(ws + p.o_exps));
    return check_launch();
}

}  // extern "C"
