// Sequence-sharded Viterbi: hmm_viterbi's chunk scan lifted across devices (included after hmm_viterbi.inc).
//
// Every rank owns one contiguous time slab of EVERY sequence, logE_slab (k, b, Ls, q) — hmm_seqshard.inc's cut, for the
// max-plus pass.  Integer max-plus is exactly associative and the maps "state at an end -> state before the start"
// compose exactly, so the slabs are one more level of the chunk scan and the result is hmm_viterbi's, bit for bit:
//
//   1. hmm_seqshard_viterbi_reduce  local: the slab's chunk operators (k_vit_reduce / k_vit_reduce_sparse), composed
//                                   into ONE operator per sequence (k_vit_scan_compose, once per level): (k,b,16,16)
//                                   int32 columns with maximum 0 + (k,b,16) int64 bases
//   2. all-gather                   the host lays the ranks' operators out (k,b,R,...)
//   3. hmm_seqshard_viterbi_apply   local: k_vit_slab_hops walks the R slab operators — every rank repeats these few
//                                   hops — and leaves the true scores entering ITS slab, the sequences' final state
//                                   and score; then the forward chunk scan from those scores, the in-chunk pass
//                                   (backpointers stay in the workspace) and the slab's map, every chunk's map composed
//   4. all-gather                   the slabs' maps, (k,b,R,16) bytes
//   5. hmm_seqshard_viterbi_path    local: the final state through the maps of the slabs behind this one
//                                   (k_vit_slab_end), the backward chunk scan and the backtrace
//
// A slab that does not begin at position 0 has no first observation (Plan::seq_start = 0): its chunk 0 is an ordinary
// chunk with an operator column per start state, entering scores, a backpointer at its step 0 and a map.  Unlike
// hmm_viterbi, which reuses one model's region for the next, the workspace holds a region per model: operators, entering
// scores, maps and backpointers of all k models have to survive from one call to the next.  Everything runs in order on
// the caller's stream: no helper streams, no batch groups.

struct SvPlan {
    VPlan v;                 // one model's b sequences of Ls positions
    size_t o_entry, o_ebase; // scores entering the slab: [b][QP] relative to their maximum, [b] maxima
    size_t o_hstart, o_hbase;// scores entering every slab, as the hops over the R slab operators record them: [b][R][QP], [b][R]
    size_t region, total;    // bytes per model, k regions
};

static int make_svplan(int k, int b, int Ls, int q, int R, SvPlan *sp) {
    if (q > QP) return HMM_ERR_Q_UNSUPPORTED;
    if (R < 1) return HMM_ERR_BAD_ARGUMENT;
    if (k < 1 || b < 1 || Ls < 1 || q < 1 || (long long)k * b > (1ll << 24)) return HMM_ERR_BAD_SHAPE;
    int rc = make_vplan(b, Ls, q, &sp->v);
    if (rc) return rc;
    size_t off = sp->v.total;
    sp->o_entry = off;  off = align_up(off + (size_t)b * QP * sizeof(int));
    sp->o_ebase = off;  off = align_up(off + (size_t)b * sizeof(long long));
    sp->o_hstart = off; off = align_up(off + (size_t)b * R * QP * sizeof(int));
    sp->o_hbase = off;  off = align_up(off + (size_t)b * R * sizeof(long long));
    sp->region = off;
    sp->total = off * (size_t)k;
    return HMM_OK;
}

// the plan that makes ONE group of all C chunks (or, with C = G, of all G groups) of a sequence
static Plan sv_whole(const Plan &p, int C) {
    Plan w = p;
    w.C = C;
    w.G = 1;
    w.gsize = C;
    return w;
}

// One sequence per block, 16 lanes, lane = state: k_vit_scan_fwd's hops over the R slab operators [seq][slab].  Slab 0's
// columns all hold the scores after it (k_vit_reduce's convention for a chunk that starts its sequence).  Leaves the
// scores entering slab r where k_vit_scan_inner reads a group's entering scores, and the sequence's final state and score.
__global__ __launch_bounds__(64) void k_vit_slab_hops(const int *__restrict__ all_vops, const long long *__restrict__ all_vbases,
                                                      int *__restrict__ hstart, long long *__restrict__ hbase,
                                                      int *__restrict__ entry, long long *__restrict__ ebase,
                                                      int *__restrict__ final_state, double *__restrict__ score,
                                                      int q, int R, int r) {
    const int seq = blockIdx.x;
    const int i = threadIdx.x;
    if (i >= 16) return;
    const size_t chain0 = (size_t)seq * R;
    long long d = (i < q) ? (long long)all_vops[chain0 * QP * QP + i * QP + 0] + all_vbases[chain0 * QP + 0] : 0;
    d = vit_hops(all_vops, all_vbases, hstart, hbase, chain0, 0, R, d, i, q);
    vit_final(d, i, q, seq, final_state, score);
    if (r > 0) {                                             // (this lane's own stores of the hop into slab r)
        entry[(size_t)seq * QP + i] = hstart[(chain0 + r) * QP + i];
        if (i == 0) ebase[seq] = hbase[chain0 + r];
    }
}

// state at this slab's last position: the final state through the maps of the slabs behind it
__global__ void k_vit_slab_end(const unsigned char *__restrict__ all_origins, const int *__restrict__ final_state,
                               int *__restrict__ sfinal, int nb, int R, int r) {
    const int seq = blockIdx.x * blockDim.x + threadIdx.x;
    if (seq >= nb) return;
    int s = final_state[seq] & 15;
    for (int c = R - 1; c > r; --c) s = all_origins[((size_t)seq * R + c) * QP + s] & 15;
    sfinal[seq] = s;
}

extern "C" {

int hmm_seqshard_viterbi_max_states(void) { return QP; }

size_t hmm_seqshard_viterbi_workspace_bytes(int k, int b, int Ls, int q, int R) {
    SvPlan sp;
    if (make_svplan(k, b, Ls, q, R, &sp)) return 0;
    return sp.total;
}

int hmm_seqshard_viterbi_reduce(const float *logA, const float *logpi, const float *logE_slab, int k, int b, int Ls, int q,
                                int seq_start, int R, int *slab_vop, long long *slab_vbase, void *workspace,
                                size_t workspace_bytes, void *stream) {
    SvPlan sp;
    int rc = make_svplan(k, b, Ls, q, R, &sp);
    if (rc) return rc;
    if (!logA || !logpi || !logE_slab || !slab_vop || !slab_vbase || !workspace) return HMM_ERR_NULL_POINTER;
    if (workspace_bytes < sp.total || ((uintptr_t)workspace & 255)) return HMM_ERR_WORKSPACE;
    VPlan v = sp.v;
    v.p.seq_start = seq_start ? 1 : 0;
    const Plan &p = v.p;
    hipStream_t st = (hipStream_t)stream;
    const int force_generic = opt(HMM_OPT_FORCE_DENSE) == 1 ? 1 : 0;
    const bool two = p.G > 0 && opt(HMM_OPT_SCAN2) != 0;
    for (int m = 0; m < k; ++m) {                            // one model per launch, as in hmm_viterbi
        char *ws = (char *)workspace + (size_t)m * sp.region;
        VModel *model = (VModel *)(ws + v.o_model);
        hipLaunchKernelGGL(k_vit_prep, dim3(1), dim3(64), 0, st, logA + (size_t)m * q * q, logpi + (size_t)m * q, model, q,
                           force_generic);
        vit_launch_reduce(logE_slab + (size_t)m * b * Ls * q, v, ws, model, q, st);
        // all chunk operators of a sequence -> one: groups first (they stay for step 3), then the groups
        const int *ops = (const int *)(ws + v.o_vops);
        const long long *bases = (const long long *)(ws + v.o_vbase);
        int nops = p.C;
        if (two) {
            const long long nwv = (long long)p.NB * p.G;
            hipLaunchKernelGGL(k_vit_scan_compose, dim3((unsigned)((nwv + 3) / 4)), dim3(256), 0, st, ops, bases,
                               (int *)(ws + v.o_gvops), (long long *)(ws + v.o_gvbase), p);
            ops = (const int *)(ws + v.o_gvops);
            bases = (const long long *)(ws + v.o_gvbase);
            nops = p.G;
        }
        hipLaunchKernelGGL(k_vit_scan_compose, dim3((unsigned)((p.NB + 3) / 4)), dim3(256), 0, st, ops, bases,
                           slab_vop + (size_t)m * b * QP * QP, slab_vbase + (size_t)m * b * QP, sv_whole(p, nops));
    }
    return check_launch();
}

int hmm_seqshard_viterbi_apply(const float *logA, const float *logpi, const float *logE_slab, int k, int b, int Ls, int q,
                               int seq_start, const int *all_vops, const long long *all_vbases, int R, int r,
                               unsigned char *slab_origin, int *final_state, double *score, void *workspace,
                               size_t workspace_bytes, void *stream) {
    SvPlan sp;
    int rc = make_svplan(k, b, Ls, q, R, &sp);
    if (rc) return rc;
    if (r < 0 || r >= R || (seq_start != 0) != (r == 0)) return HMM_ERR_BAD_ARGUMENT;
    if (!logA || !logpi || !logE_slab || !all_vops || !all_vbases || !slab_origin || !final_state || !score || !workspace)
        return HMM_ERR_NULL_POINTER;
    if (workspace_bytes < sp.total || ((uintptr_t)workspace & 255)) return HMM_ERR_WORKSPACE;
    VPlan v = sp.v;
    v.p.seq_start = seq_start ? 1 : 0;
    const Plan &p = v.p;
    hipStream_t st = (hipStream_t)stream;
    const int force_generic = opt(HMM_OPT_FORCE_DENSE) == 1 ? 1 : 0;
    const bool two = p.G > 0 && opt(HMM_OPT_SCAN2) != 0;
    for (int m = 0; m < k; ++m) {
        char *ws = (char *)workspace + (size_t)m * sp.region;
        VModel *model = (VModel *)(ws + v.o_model);
        // (the quantised model is step 1's; formed again so that this call reads nothing of it but the operators)
        hipLaunchKernelGGL(k_vit_prep, dim3(1), dim3(64), 0, st, logA + (size_t)m * q * q, logpi + (size_t)m * q, model, q,
                           force_generic);
        const int *vops = (const int *)(ws + v.o_vops);
        const long long *vbase = (const long long *)(ws + v.o_vbase);
        int *dstart = (int *)(ws + v.o_dstart);
        long long *dbase = (long long *)(ws + v.o_dbase);
        int *entry = (int *)(ws + sp.o_entry);
        long long *ebase = (long long *)(ws + sp.o_ebase);
        hipLaunchKernelGGL(k_vit_slab_hops, dim3(p.NB), dim3(64), 0, st, all_vops + (size_t)m * b * R * QP * QP,
                           all_vbases + (size_t)m * b * R * QP, (int *)(ws + sp.o_hstart), (long long *)(ws + sp.o_hbase),
                           entry, ebase, final_state + (size_t)m * b, score + (size_t)m * b, q, R, r);
        // the local chunk scan from the entering scores: the whole sequence as one group (single level), or the groups
        // as one group and then the chunks of every group
        if (!two) {
            hipLaunchKernelGGL(k_vit_scan_inner, dim3(p.NB), dim3(64), 0, st, vops, vbase, (const int *)entry,
                               (const long long *)ebase, dstart, dbase, sv_whole(p, p.C));
        } else {
            int *gdstart = (int *)(ws + v.o_gdstart);
            long long *gdbase = (long long *)(ws + v.o_gdbase);
            hipLaunchKernelGGL(k_vit_scan_inner, dim3(p.NB), dim3(64), 0, st, (const int *)(ws + v.o_gvops),
                               (const long long *)(ws + v.o_gvbase), (const int *)entry, (const long long *)ebase, gdstart,
                               gdbase, sv_whole(p, p.G));
            hipLaunchKernelGGL(k_vit_scan_inner, dim3((unsigned)((long long)p.NB * p.G)), dim3(64), 0, st, vops, vbase,
                               (const int *)gdstart, (const long long *)gdbase, dstart, dbase, p);
        }
        vit_launch_apply(logE_slab + (size_t)m * b * Ls * q, v, ws, model, q, st);
        // the slab's map: every chunk's map composed, chunk 0 included (the groups' maps stay for step 5)
        const unsigned char *maps = (const unsigned char *)(ws + v.o_forig);
        int nmaps = p.C;
        if (two) {
            const long long nwv = (long long)p.NB * p.G;
            hipLaunchKernelGGL(k_vit_bwd_compose<false>, dim3((unsigned)((nwv * QP + 255) / 256)), dim3(256), 0, st, maps,
                               (unsigned char *)(ws + v.o_gforig), p);
            maps = (const unsigned char *)(ws + v.o_gforig);
            nmaps = p.G;
        }
        hipLaunchKernelGGL(k_vit_bwd_compose<true>, dim3((unsigned)((p.NB * QP + 255) / 256)), dim3(256), 0, st, maps,
                           slab_origin + (size_t)m * b * QP, sv_whole(p, nmaps));
    }
    return check_launch();
}

int hmm_seqshard_viterbi_path(int k, int b, int Ls, int q, const unsigned char *all_origins, const int *final_state, int R,
                              int r, int32_t *path, void *workspace, size_t workspace_bytes, void *stream) {
    SvPlan sp;
    int rc = make_svplan(k, b, Ls, q, R, &sp);
    if (rc) return rc;
    if (r < 0 || r >= R) return HMM_ERR_BAD_ARGUMENT;
    if (!all_origins || !final_state || !path || !workspace) return HMM_ERR_NULL_POINTER;
    if (workspace_bytes < sp.total || ((uintptr_t)workspace & 255)) return HMM_ERR_WORKSPACE;
    const VPlan &v = sp.v;
    const Plan &p = v.p;
    hipStream_t st = (hipStream_t)stream;
    for (int m = 0; m < k; ++m) {
        char *ws = (char *)workspace + (size_t)m * sp.region;
        hipLaunchKernelGGL(k_vit_slab_end, dim3((p.NB + 63) / 64), dim3(64), 0, st, all_origins + (size_t)m * b * R * QP,
                           final_state + (size_t)m * b, (int *)(ws + v.o_sfinal), p.NB, R, r);
        vit_launch_backtrace(v, ws, path + (size_t)m * b * Ls, true, st);
    }
    return check_launch();
}

}  // extern "C"
