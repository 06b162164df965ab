// Sequence-sharded Viterbi for up to 64 states: hmm_viterbi_scan's chunk scan lifted across devices (included after
// hmm_viterbi_scan.inc, whose k_vs_* kernels it runs unchanged — hmm_seqshard_viterbi.inc's protocol with q x q
// operators in tiles of QT = 32 (q <= 32) or 64 states).
//
// Every rank owns one contiguous time slab of EVERY sequence, logE_slab (k, b, Ls, q).  Integer max-plus is exactly
// associative and the maps "state at an end -> state before the start" compose exactly, so the slabs are one more
// level of the chunk scan and the result is hmm_viterbi_scan's (= hmm_viterbi's), bit for bit:
//
//   1. hmm_seqshard_vscan_reduce  local: the slab's chunk operators (k_vs_reduce), composed into ONE operator per
//                                 sequence (k_vs_compose, once per scan level; the group operators of a two-level
//                                 scan stay in the workspace): (k,b,QT,QT) int32 columns with maximum 0 + (k,b,QT)
//                                 int64 column bases
//   2. all-gather                 the host lays the ranks' operators out (k,b,R,...)
//   3. hmm_seqshard_vscan_apply   local: k_vs_scan's top-level walk over the R slab operators (SLABS: int64 column
//                                 bases; every rank repeats these few hops) leaves the relative scores entering ITS
//                                 slab, the sequences' final state and score; then the forward chunk scan from those
//                                 scores, k_vs_apply (backpointers stay in the workspace) and the slab's map, every
//                                 chunk's map composed
//   4. all-gather                 the slabs' maps, (k,b,R,QT) bytes
//   5. hmm_seqshard_vscan_path    local: the final state through the maps of the slabs behind this one
//                                 (k_vs_slab_end), the backward chunk scan and k_vs_backtrace
//
// A slab that does not begin at position 0 has VsPlan::seq_start = 0: its chunk 0 is an ordinary chunk.  VsPlan holds
// all k models at once, so the workspace is hmm_viterbi_scan's for the slab plus the entering scores and the R
// recorded hops.  The spread bounds at the top of hmm_viterbi_scan.inc hold unchanged: a slab operator is the operator
// of a longer chunk, and the hop forms 32-bit relative column bases (in [-2^28, 0], bound (b)) from the int64 ones.
// Padding of the exchanged tensors: VS_NEG in the rows and columns of slab_vop from q on, 0 in the bases and maps.
// Everything runs in order on the caller's stream.

struct VssPlan {
    VsPlan v;                // all k models' b sequences of Ls positions
    size_t o_entry;          // scores entering the slab, relative to their maximum: [k*b][QT]
    size_t o_hops;           // scores entering every slab, as the walk over the R slab operators records them: [k*b][R][QT]
    size_t total;
};

static int make_vssplan(int k, int b, int Ls, int q, int R, VssPlan *sp) {
    if (q > MQ_MAX) return HMM_ERR_Q_UNSUPPORTED;
    if (R < 1) return HMM_ERR_BAD_ARGUMENT;
    const int rc = make_vsplan(k, b, Ls, q, &sp->v);
    if (rc) return rc;
    const size_t rows = (size_t)sp->v.NB * sp->v.QT * sizeof(int);
    size_t off = sp->v.total;
    sp->o_entry = off; off = align_up(off + rows);
    sp->o_hops = off;  off = align_up(off + rows * (size_t)R);
    sp->total = off;
    return HMM_OK;
}

// the slab's map: every chunk's (or, two levels, every group's) map composed, the first one included; all 0 for a slab
// that starts its sequences, and in the lanes from q on
__global__ void k_vs_slab_map(const unsigned char *__restrict__ maps, unsigned char *__restrict__ slab_origin, int NB,
                              int nmaps, int QT, int q, int seq_start) {
    const long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x;       // (sequence, end state)
    if (id >= (long long)NB * QT) return;
    const int j = (int)(id % QT);
    const size_t seq = (size_t)(id / QT);
    int s = 0;
    if (!seq_start && j < q) {
        s = j;
        for (int c = nmaps - 1; c >= 0; --c) s = maps[(seq * nmaps + c) * 64 + s] & 63;
    }
    slab_origin[id] = (unsigned char)s;
}

// state at this slab's last position: the final state through the maps of the slabs behind it
__global__ void k_vs_slab_end(const unsigned char *__restrict__ all_origins, const int *__restrict__ final_state,
                              int *__restrict__ sfinal, int NB, int R, int r, int QT) {
    const int seq = blockIdx.x * blockDim.x + threadIdx.x;
    if (seq >= NB) return;
    int s = final_state[seq] & (QT - 1);
    for (int c = R - 1; c > r; --c) s = all_origins[((size_t)seq * R + c) * QT + s] & (QT - 1);
    sfinal[seq] = s;
}

static void vss_prep(const float *logA, const float *logpi, const VsPlan &v, char *ws, hipStream_t st) {
    hipLaunchKernelGGL(k_mq_prep, dim3(v.k), dim3(64), 0, st, logA, (MqModel *)(ws + v.o_mq), v.q,
                       opt(HMM_OPT_FORCE_DENSE) == 1 ? 1 : 0);
    hipLaunchKernelGGL(k_vs_prep, dim3(v.k), dim3(64), 0, st, logA, logpi, (VsModel *)(ws + v.o_model), v.q);
}

static bool vss_two(const VsPlan &v) { return v.G > 0 && opt(HMM_OPT_SCAN2) != 0; }

template <int QT>
static void vss_reduce(const float *logA, const float *logpi, const float *logE, const VsPlan &v, char *ws, int *slab_vop,
                       long long *slab_vbase, hipStream_t st) {
    const dim3 wave(64);
    vss_prep(logA, logpi, v, ws, st);
    hipLaunchKernelGGL(k_vs_reduce<QT>, dim3((unsigned)v.nchains), wave, 0, st, logE, (const MqModel *)(ws + v.o_mq),
                       (const VsModel *)(ws + v.o_model), (int *)(ws + v.o_vops), (int *)(ws + v.o_vrb),
                       (long long *)(ws + v.o_vmb), v);
    // all chunk operators of a sequence -> one: groups first (they stay for step 3), then the groups
    const int *ops = (const int *)(ws + v.o_vops), *rb = (const int *)(ws + v.o_vrb);
    const long long *mb = (const long long *)(ws + v.o_vmb);
    int nops = v.C;
    if (vss_two(v)) {
        hipLaunchKernelGGL((k_vs_compose<QT, false>), dim3((unsigned)((long long)v.NB * v.G)), wave, 0, st, ops, rb, mb,
                           (int *)(ws + v.o_gvops), (int *)(ws + v.o_gvrb), (long long *)(ws + v.o_gvmb), v.q, v.C, v.G,
                           v.gsize);
        ops = (const int *)(ws + v.o_gvops); rb = (const int *)(ws + v.o_gvrb);
        mb = (const long long *)(ws + v.o_gvmb);
        nops = v.G;
    }
    hipLaunchKernelGGL((k_vs_compose<QT, true>), dim3(v.NB), wave, 0, st, ops, rb, mb, slab_vop, (int *)nullptr, slab_vbase,
                       v.q, nops, 1, nops);
}

template <int QT>
static void vss_apply(const float *logA, const float *logpi, const float *logE, const VssPlan &sp, char *ws,
                      const int *all_vops, const long long *all_vbases, int R, int r, unsigned char *slab_origin,
                      int *final_state, double *score, hipStream_t st) {
    const VsPlan &v = sp.v;
    const dim3 wave(64), seqs(v.NB);
    const int q = v.q, ss = v.seq_start;
    // (the quantised model is step 1's; formed again so that this call reads nothing of it but the operators)
    vss_prep(logA, logpi, v, ws, st);
    int *entry = (int *)(ws + sp.o_entry);
    hipLaunchKernelGGL((k_vs_scan<QT, true>), seqs, wave, 0, st, all_vops, (const int *)nullptr, all_vbases,
                       (int *)(ws + sp.o_hops), (const int *)nullptr, final_state, score, q, R, 0, 0, 1, entry, r);
    // the local chunk scan from the entering scores; it leaves final_state / score alone
    const int *vops = (const int *)(ws + v.o_vops), *vrb = (const int *)(ws + v.o_vrb);
    const long long *vmb = (const long long *)(ws + v.o_vmb);
    int *dstart = (int *)(ws + v.o_dstart);
    const bool two = vss_two(v);
    if (!two) {
        hipLaunchKernelGGL((k_vs_scan<QT, false>), seqs, wave, 0, st, vops, vrb, vmb, dstart, (const int *)entry,
                           (int *)nullptr, (double *)nullptr, q, v.C, 0, 0, ss, (int *)nullptr, 0);
    } else {
        int *gdstart = (int *)(ws + v.o_gdstart);
        hipLaunchKernelGGL((k_vs_scan<QT, false>), seqs, wave, 0, st, (const int *)(ws + v.o_gvops),
                           (const int *)(ws + v.o_gvrb), (const long long *)(ws + v.o_gvmb), gdstart, (const int *)entry,
                           (int *)nullptr, (double *)nullptr, q, v.G, 0, 0, ss, (int *)nullptr, 0);
        hipLaunchKernelGGL((k_vs_scan<QT, false>), dim3((unsigned)((long long)v.NB * v.G)), wave, 0, st, vops, vrb, vmb,
                           dstart, (const int *)gdstart, (int *)nullptr, (double *)nullptr, q, v.C, v.G, v.gsize, ss,
                           (int *)nullptr, 0);
    }
    vs_launch_apply<QT>(logE, v, ws, st);
    // the slab's map: every chunk's map composed, chunk 0 included (the groups' maps stay for step 5)
    if (two) vs_launch_group_maps(v, ws, st);
    hipLaunchKernelGGL(k_vs_slab_map, dim3((unsigned)(((long long)v.NB * QT + 255) / 256)), dim3(256), 0, st,
                       (const unsigned char *)(ws + (two ? v.o_gforig : v.o_forig)), slab_origin, v.NB, two ? v.G : v.C, QT, q,
                       ss);
}

extern "C" {

int hmm_seqshard_vscan_max_states(void) { return MQ_MAX; }

int hmm_seqshard_vscan_tile(int q) { return q < 1 || q > MQ_MAX ? 0 : (q <= 32 ? 32 : 64); }

size_t hmm_seqshard_vscan_workspace_bytes(int k, int b, int Ls, int q, int R) {
    VssPlan sp;
    if (make_vssplan(k, b, Ls, q, R, &sp)) return 0;
    return sp.total;
}

int hmm_seqshard_vscan_reduce(const float *logA, const float *logpi, const float *logE_slab, int k, int b, int Ls, int q,
                              int seq_start, int R, int *slab_vop, long long *slab_vbase, void *workspace,
                              size_t workspace_bytes, void *stream) {
    VssPlan sp;
    const int rc = make_vssplan(k, b, Ls, q, R, &sp);
    if (rc) return rc;
    if (!logA || !logpi || !logE_slab || !slab_vop || !slab_vbase || !workspace) return HMM_ERR_NULL_POINTER;
    if (workspace_bytes < sp.total || ((uintptr_t)workspace & 255)) return HMM_ERR_WORKSPACE;
    sp.v.seq_start = seq_start ? 1 : 0;
    if (sp.v.QT == 32) vss_reduce<32>(logA, logpi, logE_slab, sp.v, (char *)workspace, slab_vop, slab_vbase, (hipStream_t)stream);
    else vss_reduce<64>(logA, logpi, logE_slab, sp.v, (char *)workspace, slab_vop, slab_vbase, (hipStream_t)stream);
    return check_launch();
}

int hmm_seqshard_vscan_apply(const float *logA, const float *logpi, const float *logE_slab, int k, int b, int Ls, int q,
                             int seq_start, const int *all_vops, const long long *all_vbases, int R, int r,
                             unsigned char *slab_origin, int *final_state, double *score, void *workspace,
                             size_t workspace_bytes, void *stream) {
    VssPlan sp;
    const int rc = make_vssplan(k, b, Ls, q, R, &sp);
    if (rc) return rc;
    if (r < 0 || r >= R || (seq_start != 0) != (r == 0)) return HMM_ERR_BAD_ARGUMENT;
    if (!logA || !logpi || !logE_slab || !all_vops || !all_vbases || !slab_origin || !final_state || !score || !workspace)
        return HMM_ERR_NULL_POINTER;
    if (workspace_bytes < sp.total || ((uintptr_t)workspace & 255)) return HMM_ERR_WORKSPACE;
    sp.v.seq_start = seq_start ? 1 : 0;
    if (sp.v.QT == 32)
        vss_apply<32>(logA, logpi, logE_slab, sp, (char *)workspace, all_vops, all_vbases, R, r, slab_origin, final_state, score,
                      (hipStream_t)stream);
    else
        vss_apply<64>(logA, logpi, logE_slab, sp, (char *)workspace, all_vops, all_vbases, R, r, slab_origin, final_state, score,
                      (hipStream_t)stream);
    return check_launch();
}

int hmm_seqshard_vscan_path(int k, int b, int Ls, int q, const unsigned char *all_origins, const int *final_state, int R,
                            int r, int32_t *path, void *workspace, size_t workspace_bytes, void *stream) {
    VssPlan sp;
    const int rc = make_vssplan(k, b, Ls, q, R, &sp);
    if (rc) return rc;
    if (r < 0 || r >= R) return HMM_ERR_BAD_ARGUMENT;
    if (!all_origins || !final_state || !path || !workspace) return HMM_ERR_NULL_POINTER;
    if (workspace_bytes < sp.total || ((uintptr_t)workspace & 255)) return HMM_ERR_WORKSPACE;
    const VsPlan &v = sp.v;
    char *ws = (char *)workspace;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_vs_slab_end, dim3((v.NB + 63) / 64), dim3(64), 0, st, all_origins, final_state,
                       (int *)(ws + v.o_sfinal), v.NB, R, r, v.QT);
    vs_launch_backward(v, ws, path, vss_two(v), st);
    return check_launch();
}

}  // extern "C"
