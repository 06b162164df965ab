// hmm_grad_scan.inc — hmm_loglik_grad_scan: the log-likelihood gradients per chunk of the scan plan for every
// model of up to 64 states (included by hmm_engine.hip after hmm_postgrad.inc).
//
// hmm_loglik_grad runs per chunk for q <= 16 (hmm_grad.inc) and for the compiled 29-state topology
// (hmm_postgrad_chunked.inc: k_pc_values + k_pc_llgrad on hmm_scan_rows.inc's plan); every other model of 17..64 states
// walks two whole-sequence sweeps, one wave per sequence (hmm_midq.inc): 32 waves at b = 32 x L = 9 999.  This entry
// point runs the per-chunk kernels on the scan plan of EITHER row width — rows of 32 lanes, two chunks per wave, for
// 17..32 states; rows of 64, a chunk per wave, for 33..64 — behind the dense reduces and chunk scans of
// hmm_scan_mid.inc (scan_reduce_scan<Scan32 | Scan64>):
//
//   model     k32_check / k64_check: the support must be primitive; other models keep the whole-sequence sweeps
//   sequence  the floor-transition certificate F = eps * sum_t 1 / Sg_t <= EXACT_DELTA (k_pc_llselect) and the reduces'
//             marks (a chunk operator that went through the denormal range, or survives an observation at the
//             emission floor only); flagged sequences are redone by the masked whole-sequence sweeps in the same call
//
// It is an explicit request, as hmm_viterbi_scan is: no cap on the number of sequences (scan64_wanted's 96), and
// sparse 33..64-state models stay eligible whatever the batch.  Where it is USED is hmm_loglik_grad_scan_pays'
// business — the measured rule of DESIGN 11c (tools/experiments/llgrad_scan_time.py).

// Scan64 with a model check that keeps sparse models on the chunked path for any number of sequences
struct Scan64Req : Scan64 {
    static void check(const float *A, const MidPlan &pp, float eps, char *ws, hipStream_t st) {
        hipLaunchKernelGGL(k64_check, dim3(pp.p.k), dim3(64), 0, st, A, (int *)(ws + pp.o_elig), pp.p.q, opt(HMM_OPT_EXACT),
                           eps, (int *)(ws + pp.o_nex), 1, opt(HMM_OPT_FORCE_DENSE) == 1 ? 1 : 0);
    }
};

// hmm_loglik_grad_scan_pays: sequences per call up to which the per-chunk evaluation is preferred (0: never)
// Both 0 until tools/experiments/llgrad_scan_time.py has been run on an MI355X (DESIGN 11c): the rule never sends a
// caller of hmm_loglik_grad's wrappers here on a guess.
#define GS_PAYS_MAX_SEQ32 0
#define GS_PAYS_MAX_SEQ64 0

static int gs_width(int q) { return q <= QP ? QP : (q <= Q32 ? Q32 : (q <= Q64 ? Q64 : 0)); }

// the plan of a 17..64-state call; HMM_ERR_BAD_SHAPE for what the kernels' 32-bit row offsets do not reach
static int make_gsplan(int k, int b, int L, int q, PcPlan *pc) {
    if (k < 1 || b < 1 || L < 1 || q <= QP || q > Q64) return HMM_ERR_BAD_SHAPE;
    if ((long long)L * q * (long long)sizeof(float) >= (1ll << 31) - 4096) return HMM_ERR_BAD_SHAPE;
    return make_pcplan(k, b, L, q, pc, gs_width(q));
}

extern "C" {

int hmm_loglik_grad_scan_max_states(void) { return MQ_MAX; }

int hmm_loglik_grad_scan_chunk_len(int k, int b, int L, int q) {
    if (k < 1 || b < 1 || L < 1 || q < 1 || q > MQ_MAX) return 0;
    if (q <= QP) {
        GradPlan gp;
        return make_gradplan(k, b, L, q, &gp) ? 0 : gp.p.T;
    }
    PcPlan pc;
    return make_gsplan(k, b, L, q, &pc) ? 0 : pc.p.T;
}

size_t hmm_loglik_grad_scan_workspace_bytes(int k, int b, int L, int q) {
    if (k < 1 || b < 1 || L < 1 || q < 1 || q > MQ_MAX) return 0;
    if (q <= QP) return hmm_loglik_grad_workspace_bytes(k, b, L, q);
    PcPlan pc;
    return make_gsplan(k, b, L, q, &pc) ? 0 : pc.total;
}

// Where the per-chunk evaluation measured at least 1.25 x faster than hmm_loglik_grad's own path for the shape
// (DESIGN 11c, tools/experiments/llgrad_scan_time.py): GS_PAYS_* above.
int hmm_loglik_grad_scan_pays(int k, int b, int L, int q) {
    if (k < 1 || b < 1 || L < 1 || q <= QP || q > MQ_MAX) return 0;
    if (opt(HMM_OPT_PGCHUNK) == 0) return 0;                 // the whole-sequence sweeps are asked for
    if (pc_llgrad_wanted(k, b, L, q)) return 0;              // hmm_loglik_grad already runs per chunk
    PcPlan pc;
    if (make_gsplan(k, b, L, q, &pc)) return 0;
    if (pc.p.C < 4) return 0;
    return (long long)k * b <= (q <= Q32 ? GS_PAYS_MAX_SEQ32 : GS_PAYS_MAX_SEQ64) ? 1 : 0;
}

long long hmm_loglik_grad_scan_serial_count(int k, int b, int L, int q, const void *workspace, size_t workspace_bytes) {
    if (k < 1 || b < 1 || L < 1 || q < 1) return HMM_ERR_BAD_SHAPE;
    if (q > MQ_MAX) return HMM_ERR_Q_UNSUPPORTED;
    if (q <= QP) return hmm_loglik_grad_serial_count(k, b, L, q, workspace, workspace_bytes);
    PcPlan pc;
    int rc = make_gsplan(k, b, L, q, &pc);
    if (rc) return rc;
    return pc_llgrad_serial_count_w(k, b, L, q, workspace, workspace_bytes, pc.W);
}

int hmm_loglik_grad_scan(const float *A, const float *pi, const float *E, int k, int b, int L, int q, float eps,
                         const float *grad_loglik, float *dA, float *dpi, float *dE, double *loglik, void *workspace,
                         size_t workspace_bytes, void *stream) {
    if (k < 1 || b < 1 || L < 1 || q < 1) return HMM_ERR_BAD_SHAPE;
    if (q > MQ_MAX) return HMM_ERR_Q_UNSUPPORTED;
    if (q <= QP)
        return hmm_loglik_grad(A, pi, E, k, b, L, q, eps, grad_loglik, dA, dpi, dE, loglik, workspace, workspace_bytes, stream);
    PcPlan pc;
    int rc = make_gsplan(k, b, L, q, &pc);
    if (rc) return rc;
    if (!A || !pi || !E || !dA || !dpi || !dE || !workspace) return HMM_ERR_NULL_POINTER;
    if ((rc = check_eps(eps))) return rc;
    if (workspace_bytes < pc.total || ((uintptr_t)workspace & 255)) return HMM_ERR_WORKSPACE;
    char *ws = (char *)workspace;
    hipStream_t st = (hipStream_t)stream;
    if (pc.W == Q32)
        return pc_loglik_grad_on<Scan32>(A, pi, E, k, b, L, q, eps, grad_loglik, dA, dpi, dE, loglik, ws, pc, true, st);
    return pc_loglik_grad_on<Scan64Req>(A, pi, E, k, b, L, q, eps, grad_loglik, dA, dpi, dE, loglik, ws, pc, true, st);
}

}  // extern "C"
