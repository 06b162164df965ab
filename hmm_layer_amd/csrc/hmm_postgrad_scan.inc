// hmm_postgrad_scan.inc — hmm_posterior_grad_scan: the gradient of a loss on the state posteriors per chunk of the scan
// plan for every model of up to 64 states (included by hmm_engine.hip after hmm_grad_scan.inc, whose Scan64Req and
// make_gsplan it uses).
//
// hmm_posterior_grad runs per chunk for q <= 16 and for the compiled 29-state topology (hmm_postgrad_chunked.inc);
// every other model of 17..64 states walks four whole-sequence sweeps, one workgroup per sequence (hmm_postgrad.inc):
// 32 workgroups at b = 32 x L = 9 999.  This entry point runs the per-chunk kernels of hmm_postgrad_chunked.inc —
// k_pc_values, k_pc_src, k_pc_scan, k_pc_final, templates on the row width — on the scan plan of EITHER width: rows of
// 32 lanes, two chunks per wave, for 17..32 states; rows of 64, a chunk per wave, for 33..64 — behind the reduces and
// chunk scans of hmm_scan_mid.inc (scan_reduce_scan<Scan32 | Scan64Req>), as hmm_loglik_grad_scan does for the
// log-likelihood's gradient.  Routing, all on the device and in the same call (k_pc_scan):
//
//   model     k32_check / k64_check: the support must be primitive; other models keep the whole-sequence sweeps
//   sequence  the floor-transition certificate F = eps * sum_t 1 / Sg_t <= EXACT_DELTA, in log mode the exposed-weight
//             rule (PC_LOG_EXPOSED), and the reduces' marks — risk[chain] of the dense reduces (any q up to the row
//             width: 32 and 64 states have no pad lane), the pad lane of the exponent row for the compiled 29-state
//             reduce — read as k_pc_llselect reads them
//
// Flagged sequences and the models the checks turn down are redone by the masked whole-sequence sweeps, with the
// instantiation hmm_posterior_grad itself picks for q (k_pg_*<32 | 48 | 64>): bit-identical to that call under
// HMM_OPT_PGCHUNK = 0.  Like hmm_loglik_grad_scan it is an explicit request: no cap on the number of sequences, and
// sparse 33..64-state models stay eligible whatever the batch.  Where it is USED is hmm_posterior_grad_scan_pays'
// business — the measured rule of DESIGN 12c (tools/experiments/postgrad_scan_time.py).

// hmm_posterior_grad_scan_pays: sequences per call up to which the per-chunk evaluation is preferred (0: never).
// Measured on an MI355X (DESIGN 12c): the largest batch of tools/experiments/postgrad_scan_time.py's table at which
// the scan was >= 1.25 x faster than hmm_posterior_grad for every model of the width — rows of 32: 2.09 x at 128
// sequences, 0.78 x at 512; rows of 64: 1.62 .. 1.73 x at 64, 0.88 .. 0.95 x at 128.
#define PGS_PAYS_MAX_SEQ32 128
#define PGS_PAYS_MAX_SEQ64 64

// S: Scan32 / Scan64Req; pc: make_gsplan's for S::W
template <class S>
static int pgs_launch(const float *A, const float *pi, const float *E, int k, int b, int L, int q, float eps, int mode,
                      const float *G, float *dA, float *dpi, float *dE, char *ws, const PcPlan &pc, hipStream_t st) {
    scan_reduce_scan<S>(A, pi, E, pc.mid, eps, ws, st);
    return pc_launch_w<S::W>(A, pi, E, k, b, L, q, eps, mode, PgStateG{G}, dA, dpi, dE, ws, pc, st, (const int *)(ws + pc.mid.o_risk));
}

extern "C" {

int hmm_posterior_grad_scan_max_states(void) { return MQ_MAX; }

int hmm_posterior_grad_scan_chunk_len(int k, int b, int L, int q) {
    if (k < 1 || b < 1 || L < 1 || q < 1 || q > MQ_MAX) return 0;
    PcPlan pc;
    if (q <= QP)                                             // hmm_posterior_grad's: its plan's, or the sequence as one chunk
        return pc_wanted(k, b, L, q) ? (make_pcplan(k, b, L, q, &pc) ? 0 : pc.p.T) : L;
    return make_gsplan(k, b, L, q, &pc) ? 0 : pc.p.T;
}

size_t hmm_posterior_grad_scan_workspace_bytes(int k, int b, int L, int q) {
    if (k < 1 || b < 1 || L < 1 || q < 1 || q > MQ_MAX) return 0;
    if (q <= QP) return hmm_posterior_grad_workspace_bytes(k, b, L, q);
    PcPlan pc;
    return make_gsplan(k, b, L, q, &pc) ? 0 : pc.total;
}

// Where the per-chunk evaluation measured at least 1.25 x faster than hmm_posterior_grad's own path for the shape
// (DESIGN 12c, tools/experiments/postgrad_scan_time.py): PGS_PAYS_* above.
int hmm_posterior_grad_scan_pays(int k, int b, int L, int q) {
    if (k < 1 || b < 1 || L < 1 || q <= QP || q > MQ_MAX) return 0;
    if (opt(HMM_OPT_PGCHUNK) == 0) return 0;                 // the whole-sequence sweeps are asked for
    if (pc_wanted(k, b, L, q)) return 0;                     // hmm_posterior_grad already runs per chunk
    PcPlan pc;
    if (make_gsplan(k, b, L, q, &pc)) return 0;
    if (pc.p.C < 4) return 0;
    return (long long)k * b <= (q <= Q32 ? PGS_PAYS_MAX_SEQ32 : PGS_PAYS_MAX_SEQ64) ? 1 : 0;
}

long long hmm_posterior_grad_scan_serial_count(int k, int b, int L, int q, const void *workspace, size_t workspace_bytes) {
    if (k < 1 || b < 1 || L < 1 || q < 1) return HMM_ERR_BAD_SHAPE;
    if (q > MQ_MAX) return HMM_ERR_Q_UNSUPPORTED;
    if (q <= QP) return hmm_posterior_grad_serial_count(k, b, L, q, workspace, workspace_bytes);
    PcPlan pc;
    int rc = make_gsplan(k, b, L, q, &pc);
    if (rc) return rc;
    return pc_llgrad_serial_count_w(k, b, L, q, workspace, workspace_bytes, pc.W);      // (need[] of the same plan)
}

int hmm_posterior_grad_scan(const float *A, const float *pi, const float *E, int k, int b, int L, int q, float eps,
                            int mode, const float *grad_out, float *dA, float *dpi, float *dE, void *workspace,
                            size_t workspace_bytes, void *stream) {
    if (k < 1 || b < 1 || L < 1 || q < 1) return HMM_ERR_BAD_SHAPE;
    if (q > MQ_MAX) return HMM_ERR_Q_UNSUPPORTED;
    if (q <= QP)
        return hmm_posterior_grad(A, pi, E, k, b, L, q, eps, mode, grad_out, dA, dpi, dE, workspace, workspace_bytes, stream);
    if (mode != HMM_POST_PROB && mode != HMM_POST_LOG) return HMM_ERR_BAD_ARGUMENT;
    if (!A || !pi || !E || !grad_out || !dA || !dpi || !dE || !workspace) return HMM_ERR_NULL_POINTER;
    if (check_eps(eps)) return HMM_ERR_BAD_ARGUMENT;
    PcPlan pc;
    int rc = make_gsplan(k, b, L, q, &pc);
    if (rc) return rc;
    if (workspace_bytes < pc.total || ((uintptr_t)workspace & 255)) return HMM_ERR_WORKSPACE;
    char *ws = (char *)workspace;
    hipStream_t st = (hipStream_t)stream;
    if (pc.W == Q32)
        return pgs_launch<Scan32>(A, pi, E, k, b, L, q, eps, mode, grad_out, dA, dpi, dE, ws, pc, st);
    return pgs_launch<Scan64Req>(A, pi, E, k, b, L, q, eps, mode, grad_out, dA, dpi, dE, ws, pc, st);
}

}  // extern "C"
