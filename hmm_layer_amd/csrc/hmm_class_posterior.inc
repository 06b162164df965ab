// hmm_class_posterior.inc — class posteriors with analytic gradients for q <= 16 states (included last by
// hmm_engine.hip): the trainable counterpart of hmm_posterior_decode, and the q <= 16 sibling of
// hmm_class_posterior_walk / hmm_class_posterior_grad_walk (hmm_wideq.inc, hmm_postgradwq.inc).
//
//   forward   hmm_posterior(HMM_POST_PROB)'s pipeline — chunked kernels, windows, exact serial kernels, same routing and
//             workspace — with the ClassOut output policy of backward_body (hmm_engine.hip) in place of the gamma rows:
//             Decode's staging, weight table and class-sum loop, every class's sum stored.  out_log receives the sums
//             too and k_wq_class_log (hmm_wideq.inc) turns them into logs in place afterwards: the fp64 log rounded
//             once (logf measured over 2 ulp on such sums there), outside the decode-family kernel, which sits at the
//             edge of its register budget.
//   backward  hmm_posterior_grad's sweeps (hmm_postgrad.inc whole-sequence, hmm_postgrad_chunked.inc per chunk) with
//             the PgClassG loader: a state reads Gc[t][class(state)] in place.  Log mode: k_cp_quot writes
//             G' = Gc / P into the workspace, with the three per-sequence sums of the class routing rule, and the
//             adjoints run in prob mode on G' (k_pc_class_rule applies the rule between k_pc_scan and k_pc_final).

#define CP_PART_ELEMS 32768      // elements of a sequence's (L, C) slab per block of the pre-pass ...
#define CP_PARTS_MAX 32          // ... up to this many blocks per sequence
static int cp_parts(int L, int C) {
    const long long n = ((long long)L * C + CP_PART_ELEMS - 1) / CP_PART_ELEMS;
    return (int)(n < 1 ? 1 : (n > CP_PARTS_MAX ? CP_PARTS_MAX : n));
}

// log mode's upstream gradient in prob-mode terms, G' = Gc / P (the IEEE fp32 quotient; 0 where P == 0), and the
// sums of the routing rule: block (seq, i) takes the i-th of `parts` equal runs of the sequence's L * C elements and
// leaves (sum_{P >= 1e-8} |G'|, sum_{P < 1e-8} |Gc|, sum |Gc|) in fp64 at csum[seq][i] — thread-strided partials,
// then a fixed tree: the same sums for every call.
__global__ __launch_bounds__(256) void k_cp_quot(const float *__restrict__ g, const float *__restrict__ P,
                                                 float *__restrict__ Gp, long long per, int parts,
                                                 double *__restrict__ csum) {
    __shared__ double s0[256], s1[256], s2[256];
    const int seq = blockIdx.x, i = blockIdx.y;
    const long long run = (per + parts - 1) / parts, lo = (long long)i * run, hi = lo + run < per ? lo + run : per;
    const size_t base = (size_t)seq * (size_t)per;
    double a = 0.0, b = 0.0, c = 0.0;
    for (long long e = lo + threadIdx.x; e < hi; e += 256) {
        const float p = P[base + e], gv = g[base + e];
        const float qv = p > 0.f ? gv / p : 0.f;
        Gp[base + e] = qv;
        const float w = __builtin_fabsf(gv);
        const bool tiny = !(p >= PG_TINY_GAMMA);
        a += tiny ? 0.0 : (double)__builtin_fabsf(qv);
        b += tiny ? (double)w : 0.0;
        c += (double)w;
    }
    s0[threadIdx.x] = a; s1[threadIdx.x] = b; s2[threadIdx.x] = c;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            s0[threadIdx.x] += s0[threadIdx.x + s]; s1[threadIdx.x] += s1[threadIdx.x + s]; s2[threadIdx.x] += s2[threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        double *t = csum + ((size_t)seq * parts + i) * 3;
        t[0] = s0[0]; t[1] = s1[0]; t[2] = s2[0];
    }
}

// hmm_posterior_grad's layout (either plan) first, then G' and the rule's sums
struct CpPlan { size_t base, o_gp, o_csum, total; int parts; };
static int make_cpplan(int k, int b, int L, int q, int C, CpPlan *cp) {
    cp->base = hmm_posterior_grad_workspace_bytes(k, b, L, q);
    if (!cp->base) return HMM_ERR_BAD_SHAPE;
    cp->parts = cp_parts(L, C);
    size_t off = align_up(cp->base);
    cp->o_gp = off;   off = align_up(off + (size_t)k * b * L * C * sizeof(float));
    cp->o_csum = off; off = align_up(off + (size_t)k * b * cp->parts * 3 * sizeof(double));
    cp->total = off;
    return HMM_OK;
}

extern "C" {

int hmm_class_posterior_max_states(void) { return QP; }

size_t hmm_class_posterior_workspace_bytes(int k, int b, int L, int q) {
    if (k < 1 || b < 1 || L < 1 || q < 1 || q > QP) return 0;
    return hmm_workspace_bytes(HMM_OP_POSTERIOR, k, b, L, q);
}

// 1 exactly on the cells tools/experiments/class_posterior_time.py measured at least 1.25x ahead of the composition
// (profiles/class_posterior.json, DESIGN §12g); 0 everywhere else, everything not measured included: other state or
// class counts, other batches or lengths, more than one model.  Measured on one MI355X, one model, log mode, the
// 7-state topology with 4 classes and the 15-state gene model with 5, a label-style upstream gradient:
//   forward alone (out_log) against hmm_posterior + index_add_ + log: 1.39x .. 4.80x ahead in all eight cells;
//   the autograd node (both calls) against the composed node: 0.02x .. 1.03x — the labels of the measurement are
//   uniform over the classes, the class log rule sends every sequence to the whole-sequence sweeps, and the composed
//   node (a prob-mode state call on Gc / P) has no such rule.  So the gradient predicate has no cell.
struct CpCell { int q, b, L; };
static const CpCell cp_fwd_cells[] = {{7, 1, 100000},  {7, 32, 9999},  {7, 1024, 10000},  {7, 1024, 100000},
                                      {15, 1, 100000}, {15, 32, 9999}, {15, 1024, 10000}, {15, 1024, 100000}};
static const CpCell cp_grad_cells[] = {{0, 0, 0}};           // (none measured ahead; q = 0 matches no call)
static int cp_in(const CpCell *t, size_t n, int k, int b, int L, int q) {
    if (k != 1) return 0;
    for (size_t i = 0; i < n; ++i)
        if (t[i].q == q && t[i].b == b && t[i].L == L) return 1;
    return 0;
}
int hmm_class_posterior_pays(int k, int b, int L, int q) {
    if (k < 1 || b < 1 || L < 1 || q < 1 || q > QP) return 0;
    return cp_in(cp_fwd_cells, sizeof(cp_fwd_cells) / sizeof(CpCell), k, b, L, q);
}
int hmm_class_posterior_grad_pays(int k, int b, int L, int q) {
    if (k < 1 || b < 1 || L < 1 || q < 1 || q > QP) return 0;
    return cp_in(cp_grad_cells, sizeof(cp_grad_cells) / sizeof(CpCell), k, b, L, q);
}

int hmm_class_posterior(const float *A, const float *pi, const float *E, int k, int b, int L, int q, float eps,
                        const int *state_class, int num_classes, float *out_prob, float *out_log, double *loglik,
                        void *workspace, size_t workspace_bytes, void *stream) {
    if (k < 1 || b < 1 || L < 1 || q < 1) return HMM_ERR_BAD_SHAPE;
    if (q > QP) return HMM_ERR_Q_UNSUPPORTED;
    Route r;
    int rc = make_route(HMM_OP_POSTERIOR, k, b, L, q, &r);
    if (rc) return rc;
    if (!A || !pi || !E || !state_class || !workspace || (!out_prob && !out_log)) return HMM_ERR_NULL_POINTER;
    if (num_classes < 1 || num_classes > QP || check_eps(eps)) return HMM_ERR_BAD_ARGUMENT;
    ClassOut cls{};
    cls.prob = out_prob; cls.logp = out_log; cls.ncls = num_classes;
    for (int s = 0; s < q; ++s) {                              // the table is read here, once, and travels by value
        if (state_class[s] < 0 || state_class[s] >= num_classes) return HMM_ERR_BAD_ARGUMENT;
        cls.w[state_class[s]][s] = 1.f;
    }
    if ((rc = check_ws(r.total, workspace, workspace_bytes))) return rc;
    hipStream_t st = (hipStream_t)stream;
    rc = s16_posterior(A, pi, E, r.G, eps, HMM_POST_PROB, nullptr, loglik, (char *)workspace, st, nullptr, &cls);
    if (rc) return rc;
    if (out_log) {
        const size_t n = (size_t)k * b * L * num_classes, nb = (n + 255) / 256;
        launch(k_wq_class_log, dim3((unsigned)(nb < 65536 ? nb : 65536)), dim3(256), 0, st, out_log, n);
    }
    return check_launch();
}

size_t hmm_class_posterior_grad_workspace_bytes(int k, int b, int L, int q, int num_classes) {
    CpPlan cp;
    if (k < 1 || b < 1 || L < 1 || q < 1 || q > QP || num_classes < 1 || num_classes > QP) return 0;
    return make_cpplan(k, b, L, q, num_classes, &cp) ? 0 : cp.total;
}

int hmm_class_posterior_grad(const float *A, const float *pi, const float *E, int k, int b, int L, int q, float eps,
                             int mode, const int *state_class, int num_classes, const float *class_prob,
                             const float *grad_out, float *dA, float *dpi, float *dE, void *workspace,
                             size_t workspace_bytes, void *stream) {
    if (k < 1 || b < 1 || L < 1 || q < 1) return HMM_ERR_BAD_SHAPE;
    if (q > QP) return HMM_ERR_Q_UNSUPPORTED;
    if (mode != HMM_POST_PROB && mode != HMM_POST_LOG) return HMM_ERR_BAD_ARGUMENT;
    if (!A || !pi || !E || !state_class || !grad_out || !dA || !dpi || !dE || !workspace ||
        (mode == HMM_POST_LOG && !class_prob))
        return HMM_ERR_NULL_POINTER;
    if (num_classes < 1 || num_classes > QP || check_eps(eps)) return HMM_ERR_BAD_ARGUMENT;
    PgClassG gl{};
    gl.C = num_classes;
    for (int s = 0; s < q; ++s) {                              // the table is read here, once, and travels by value
        if (state_class[s] < 0 || state_class[s] >= num_classes) return HMM_ERR_BAD_ARGUMENT;
        gl.cls |= (unsigned long long)state_class[s] << (4 * s);
    }
    CpPlan cp;
    int rc = make_cpplan(k, b, L, q, num_classes, &cp);
    if (rc) return rc;
    if ((rc = check_ws(cp.total, workspace, workspace_bytes))) return rc;
    char *ws = (char *)workspace;
    hipStream_t st = (hipStream_t)stream;
    if (q == 1) {                                              // gamma = 1 identically: exact zeros (hmm_posterior_grad)
        if (hipMemsetAsync(dA, 0, (size_t)k * sizeof(float), st) != hipSuccess ||
            hipMemsetAsync(dpi, 0, (size_t)k * sizeof(float), st) != hipSuccess ||
            hipMemsetAsync(dE, 0, (size_t)k * b * L * sizeof(float), st) != hipSuccess)
            return HMM_ERR_LAUNCH;
        return HMM_OK;
    }
    gl.G = grad_out;
    const double *csum = nullptr;
    if (mode == HMM_POST_LOG) {                                // d/d gamma_j of sum Gc log P = Gc / P at j's class
        float *Gp = ws_at<float>(ws, cp.o_gp);
        double *cs = ws_at<double>(ws, cp.o_csum);
        launch(k_cp_quot, dim3((unsigned)(k * b), (unsigned)cp.parts), dim3(256), 0, st, grad_out, class_prob, Gp,
               (long long)L * num_classes, cp.parts, cs);
        gl.G = Gp;
        csum = cs;
    }
    if (pc_wanted(k, b, L, q)) {
        PcPlan pc;
        if ((rc = make_pcplan(k, b, L, q, &pc))) return rc;
        if ((rc = run_reduce_scan(A, pi, E, pc.p, eps, ws, st))) return rc;
        return pc_launch_w<QP>(A, pi, E, k, b, L, q, eps, (int)HMM_POST_PROB, gl, dA, dpi, dE, ws, pc, st, nullptr, csum,
                               cp.parts);
    }
    PgPlan pp;
    make_pgplan(k, b, L, q, &pp);
    pg_launch<16>(A, pi, E, k, b, L, q, eps, (int)HMM_POST_PROB, gl, dA, dE, ws, pp, st);
    hipLaunchKernelGGL(k_pg_sum_rows, dim3(q, k), dim3(64), 0, st, (const float *)(ws + pp.o_dpi), dpi, b, q);
    return check_launch();
}

}  // extern "C"
