// hmm_emitter_grad.inc — backward of the fused gene emitters (hmm_emitter.inc), included by
// hmm_engine.hip after it.  Replaces autograd through GenePredHMMEmitter.forward
// (hmm_layer/gene_pred_hmm_emitter.py:231-277 over :93-121 and kmer.make_k_mers, hmm_layer/kmer.py:3-47),
// which keeps two (b,L,64) 3-mer tensors and a (b,L,2,q) product alive until backward().  With
//
//   emit[p,j] = sum_c x[p,c] * B[state_row[j], c],   E[p,j] = emit[p,j] * (cod[p,j] + add)
//
// and G = dL/dE, H[p,j] = G[p,j] * (cod[p,j] + add):
//
//   dx[p,c] = sum_j H[p,j] * B[state_row[j], c]                   (c < s; the five nucleotide columns are 0:
//                                                                  one-hot nucleotides are data)
//   dB[r,c] = sum_p sum_{j: state_row[j] = r} H[p,j] * x[p,c]
//
// cod depends on the nucleotide columns only and is recomputed exactly as in the forward (the window
// tables, the code words, the generic path: em_build_tables, em_classify, em_scale_tile), so nothing per
// position is kept between forward and backward but x itself.
//
// Both kernels are shells round emg_group_pass, the backward of one group of up to 16 NT states over all the runs of
// a wave, and emg_write_partial; the run walker (em_walk), the flat flush (em_flush_flat) and the clamped table reads
// (em_row, em_codon) are hmm_emitter.inc's.
//
// Shape of a group pass: the forward's.  A wave owns runs of run_len positions and walks 16-position tiles.
//   H    em_scale_tile applied to the dE tile loaded in the D layout (lane (g, n): state 16 nt + n at
//        positions 4g..4g+3) writes H into the wave-private LDS stage, rows = positions, stride 16 NT + 4.
//   dB   H read back in the D layout is the A operand (rows = states, K = positions) of
//        dBexp (16 NT x 16 KT) += H^T X, X loaded as the B operand (lane (g, n): class 16 kt + n of positions
//        4g..4g+3).  The NT x KT f4 accumulators live over all the runs of the wave.
//   dx   H read back with 16-byte loads in the A-operand layout (lane (g, m): states 4g..4g+3 of position m)
//        times Bexp, constant in B-operand registers; the result goes through the same stage (stride s + 5,
//        nucleotide columns zero) and leaves in 16-byte stores, (s + 5) x 64 contiguous bytes per tile.
// Entries of the stage that em_scale_tile does not write (states >= q, positions >= b L) are masked to 0
// when read back.
//
// dB is summed in a fixed order, so repeated calls are bit-identical (the grid depends on b L only):
//   1. the waves of a block add their accumulators into one LDS copy of dBexp, wave 0 first;
//   2. states are folded into kernel rows in ascending state order (state_row, clamped into 0..rows-1);
//   3. the block writes its (rows, s) partial into the workspace;
//   4. k_gene_emissions_grad_sum adds the block partials in block order in fp64 and writes fp32 dB.
// dB is written whole by the call: the caller does not zero it.
//
// hmm_gene_emissions_grad (q <= 64, rows <= 32): one group pass over runs of EM_RUN positions.
// Compiler figures (gfx950, hipcc -O3), <NT, KT>; tables = 2 max(nc,1) x 2 KiB (36 KiB for the gene model's nc = 9):
//   <1, 1>  (q <= 16, s <= 16)   128 VGPRs (the launch bound's cap), 8 B scratch (one spilled register),
//                                LDS per block = tables + 8 stages of 1344 B + 1 KiB  (48 640 B)
//   <4, 2>  (everything else)    236 VGPRs, no scratch, LDS per block = tables + 8 stages of 4352 B + 8 KiB  (79 872 B)
//
// hmm_gene_emissions_grad_wide (up to 256 states and 256 rows): <4, 2> group passes over groups of 64 states, the group
// OUTERMOST (group -> the wave's runs -> the run's 16-position tiles).  Per group a wave holds that group's Bexp slice
// in B-operand registers (bx[4][2]) and its 32 accumulator registers of dBexp (acc[4][2]); neither would fit for
// four groups at once.
//   dx   group 0 writes the tile, every later group adds its product to what is there.  The tile leaves through the
//        stage in 16-byte pieces, piece -> lane fixed, so the same lane reads back what it wrote one group earlier:
//        plain program order of one thread, no atomics, and the sum over groups runs in ascending group order whatever
//        the grid.
//   dB   after a group's runs the waves of the workgroup add acc into rows 64 grp .. of the LDS copy of dBexp
//        (q x 32), wave 0 first; the fold and the partials follow after the last group.
// Cost of the order: x's class columns and the nucleotides are read once per group (s + 5 floats per position against
// the 64 floats of dE a group reads), and dx is read and written once more per further group.  With one run per wave
// (b L <= 8 runs x grid) a run's dx (at most 1024 (s + 5) floats) is still in L2 when the next group comes for it.
// Runs are emw_run_len(b L) positions long (1024, shorter where b L would leave CUs idle): a function of b L alone, so
// the summation order of dB is fixed per shape.
// The grid is min(runs / 8, 1024, 16 MiB / (rows s 4)) workgroups, so the partials stay within 16 MiB; the workspace
// is sized for that cap and does not depend on b L.
// LDS per workgroup: tables 2 max(nc,1) x 2 KiB + 8 stages of 16 max(68, s + 5) floats + dBexp 64 ngrp x 128 B:
// 36 864 + 34 816 + 8192 ngrp bytes for nc = 9, 104 448 B at 256 states.  One workgroup per CU.
// Compiler figures (gfx950, hipcc -O3): 249 VGPRs, no scratch.

#define EMG_MAXBLOCKS 1024  // block partials the second kernel sums
#define EMGW_PART_BYTES ((size_t)16 << 20)

// The backward of states j0 .. j0 + min(q - j0, 16 NT) - 1 over all the runs of this wave: dx tiles out (accumulate:
// added to the dx already stored), then, with want_dB, the waves' dBexp accumulators into rows j0 .. of red in wave
// order.  T9: the built window tables; stage: this wave's; red: the workgroup's [states][16 KT].
template <int NT, int KT>
__device__ __forceinline__ void emg_group_pass(const float *__restrict__ x, long long npos, int L, int s,
                                               const float *__restrict__ B, int rows, const int *__restrict__ state_row,
                                               int nc, const int *__restrict__ state_codon, int q, int j0, int run_len,
                                               bool accumulate, float free_value, float add, float n_mass,
                                               const float *__restrict__ dE, float *dx, bool want_dB, const float *T9,
                                               float *stage, float *red, int tid) {
    constexpr int QS = 16 * NT + 4;                                // row stride of the H stage
    const int w = s + 5, ncp = nc > 0 ? nc : 1, qg = q - j0;
    const int lane = tid & 63, g = lane >> 4, n = lane & 15;
    const bool want_dx = dx != nullptr;
    // B-operand registers of the dx product: Bexp[state j0 + 16 nt + 4g + kk][class 16 kt + n]; this lane's table rows
    f4 bx[NT][KT];
    int cj[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        cj[nt] = 16 * nt + n < qg ? em_codon(state_codon, j0 + 16 * nt + n, nc) : -1;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            const int j = 16 * nt + 4 * g + kk;
            const int brow = j < qg ? em_row(state_row, j0 + j, rows) : 0;
#pragma unroll
            for (int kt = 0; kt < KT; ++kt) {
                const int cls = 16 * kt + n;
                bx[nt][kt][kk] = (j < qg && cls < s) ? B[(size_t)brow * s + cls] : 0.f;
            }
        }
    }
    const f4 zero4 = {0.f, 0.f, 0.f, 0.f};
    f4 acc[NT][KT];                                         // dBexp[state j0 + 16 nt + 4g + r][class 16 kt + n]
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int kt = 0; kt < KT; ++kt) acc[nt][kt] = zero4;
    const int npieces = 4 * w;                              // 16-byte pieces per dx tile

    struct GT { f4 v[NT]; };
    auto load_G = [&](long long Pt) {                       // the group's dE tile at Pt in the D layout, 0 outside
        GT gt;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long long pos = Pt + 4 * g + r;
                const int j = 16 * nt + n;
                gt.v[nt][r] = (pos < npos && j < qg) ? dE[pos * q + j0 + j] : 0.f;
            }
        return gt;
    };
    GT gcur;
    em_walk<0, false>(x, npos, L, s, run_len, tid, [&](long long P0) { gcur = load_G(P0); }, [&](const EmTile<0> &t) {
        const long long P = t.P;
        const GT gnx = load_G(P + 16);                      // one tile ahead
        f4 xb[KT];                                          // B operand of the dB product: x[P + 4g + r][16 kt + n]
        if (want_dB) {
#pragma unroll
            for (int kt = 0; kt < KT; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const long long pos = P + 4 * g + r;
                    const int cls = 16 * kt + n;
                    xb[kt][r] = (pos < npos && cls < s) ? x[pos * w + cls] : 0.f;
                }
        }
        em_scale_tile<NT>(gcur.v, stage, QS, cj, qg, T9, ncp, t.prev, t.cur, t.nxt, t.tb, L, P, npos, g, n, x, s, w,
                          free_value, add, n_mass);
        __builtin_amdgcn_wave_barrier();                    // stage is wave-private: LDS ops of a wave execute in order
        f4 Hd[NT], Ha[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            Ha[nt] = *reinterpret_cast<const f4 *>(stage + n * QS + 16 * nt + 4 * g);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float v = stage[(4 * g + r) * QS + 16 * nt + n];
                Hd[nt][r] = (P + 4 * g + r < npos && 16 * nt + n < qg) ? v : 0.f;
                Ha[nt][r] = (P + n < npos && 16 * nt + 4 * g + r < qg) ? Ha[nt][r] : 0.f;
            }
        }
        __builtin_amdgcn_wave_barrier();
        if (want_dB) {
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int kt = 0; kt < KT; ++kt) acc[nt][kt] = mfma4v(Hd[nt], xb[kt], acc[nt][kt]);
        }
        if (want_dx) {
#pragma unroll
            for (int kt = 0; kt < KT; ++kt) {
                f4 Dx = zero4;                              // dx[P + 4g + r][class 16 kt + n]
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) Dx = mfma4v(Ha[nt], bx[nt][kt], Dx);
                const int cls = 16 * kt + n;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if (cls < s) stage[(4 * g + r) * w + cls] = Dx[r];
                    if (kt == 0 && n < 5) stage[(4 * g + r) * w + s + n] = 0.f;
                }
            }
            __builtin_amdgcn_wave_barrier();
            // the tile is 64 (s + 5) contiguous bytes of dx
            em_flush_flat<false>(stage, dx + P * w, (npos - P < 16 ? npos - P : 16) * w, npieces, lane, accumulate);
            __builtin_amdgcn_wave_barrier();
        }
        gcur = gnx;
    });

    if (want_dB) {
        // waves in fixed order into the group's rows of dBexp
        for (int wv = 0; wv < EM_THREADS / 64; ++wv) {
            if ((tid >> 6) == wv) {
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                    for (int kt = 0; kt < KT; ++kt)
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            red[(j0 + 16 * nt + 4 * g + r) * (16 * KT) + 16 * kt + n] += acc[nt][kt][r];
            }
            __syncthreads();
        }
    }
}

// states of red ([q][16 KT]) into kernel rows in ascending state order: the workgroup's (rows, s) partial
template <int KT>
__device__ __forceinline__ void emg_write_partial(const float *red, const int *__restrict__ state_row, int rows, int q, int s,
                                                  float *__restrict__ part, int tid) {
    float *dst = part + (size_t)blockIdx.x * rows * s;
    for (int e = tid; e < rows * s; e += EM_THREADS) {
        const int rr = e / s, c = e - rr * s;
        float sum = 0.f;
        for (int j = 0; j < q; ++j)
            if (em_row(state_row, j, rows) == rr) sum += red[j * (16 * KT) + c];
        dst[e] = sum;
    }
}

// LDS of both kernels: [2][max(nc,1)][512] tables, 8 stages of 16 x max(16 NT + 4, s + 5) floats, dBexp [states][16 KT]
struct EmgLds { float *stage, *red; };                     // this wave's stage, the workgroup's dBexp
template <int NT>
__device__ __forceinline__ EmgLds emg_lds(float *T9, int nc, int s, int tid) {
    const int qs = 16 * NT + 4, w = s + 5, stf = 16 * (qs > w ? qs : w);
    float *base = T9 + (size_t)2 * (nc > 0 ? nc : 1) * 512;
    return {base + (size_t)(tid >> 6) * stf, base + (size_t)(EM_THREADS / 64) * stf};
}

// (second launch bound: waves per SIMD.  The one-tile variant is held to 128 VGPRs so that two blocks share a CU;
// uncapped it takes 138 and a grid of more than 256 blocks runs in two rounds)
template <int NT, int KT>
__global__ __launch_bounds__(EM_THREADS, NT == 1 ? 4 : 2) void k_gene_emissions_grad(const float *__restrict__ x, long long npos, int L, int s,
                                                                    const float *__restrict__ B,
                                                                    const int *__restrict__ state_row,
                                                                    const float *__restrict__ codon, int nc,
                                                                    const int *__restrict__ state_codon, int q, int rows,
                                                                    float free_value, float add, float n_mass,
                                                                    const float *__restrict__ dE, float *__restrict__ dx,
                                                                    float *__restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) float T9[];
    const int tid = threadIdx.x;
    const EmgLds lds = emg_lds<NT>(T9, nc, s, tid);         // dBexp: [16 NT][16 KT]
    em_build_tables(T9, codon, nc, n_mass, tid);
    for (int e = tid; e < 256 * NT * KT; e += EM_THREADS) lds.red[e] = 0.f;
    __syncthreads();
    emg_group_pass<NT, KT>(x, npos, L, s, B, rows, state_row, nc, state_codon, q, 0, EM_RUN, false, free_value, add, n_mass,
                           dE, dx, part != nullptr, T9, lds.stage, lds.red, tid);
    if (part) emg_write_partial<KT>(lds.red, state_row, rows, q, s, part, tid);
}

__global__ __launch_bounds__(EM_THREADS, 2) void k_gene_emissions_grad_wide(const float *__restrict__ x, long long npos, int L, int s,
                                                                         const float *__restrict__ B,
                                                                         const int *__restrict__ state_row,
                                                                         const float *__restrict__ codon, int nc,
                                                                         const int *__restrict__ state_codon, int q, int rows,
                                                                         float free_value, float add, float n_mass, int run_len,
                                                                         const float *__restrict__ dE, float *dx,
                                                                         float *__restrict__ part) {
    constexpr int NT = 4, KT = 2;
    extern __shared__ __attribute__((aligned(16))) float T9[];
    const int tid = threadIdx.x;
    const int ngrp = (q + 63) >> 6, qp = 64 * ngrp;
    const EmgLds lds = emg_lds<NT>(T9, nc, s, tid);         // dBexp: [qp][16 KT]
    em_build_tables(T9, codon, nc, n_mass, tid);
    if (part)
        for (int e = tid; e < qp * 16 * KT; e += EM_THREADS) lds.red[e] = 0.f;
    __syncthreads();
#pragma unroll 1
    for (int grp = 0; grp < ngrp; ++grp)
        emg_group_pass<NT, KT>(x, npos, L, s, B, rows, state_row, nc, state_codon, q, 64 * grp, run_len, grp > 0, free_value,
                               add, n_mass, dE, dx, part != nullptr, T9, lds.stage, lds.red, tid);
    if (part) emg_write_partial<KT>(lds.red, state_row, rows, q, s, part, tid);
}

// dB[e] = sum over the block partials in block order, fp64
__global__ __launch_bounds__(64) void k_gene_emissions_grad_sum(const float *__restrict__ part, int nblk, int nel,
                                                                float *__restrict__ dB) {
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (e >= nel) return;
    double sum = 0.0;
    for (int k = 0; k < nblk; ++k) sum += (double)part[(size_t)k * nel + e];
    dB[e] = (float)sum;
}

// workgroups = block partials.  64-state: one per 8 runs of EM_RUN, at most EMG_MAXBLOCKS.  Wide: at most EMG_MAXBLOCKS
// and at most 16 MiB of (rows, s) partials.
static long long emg_blocks(long long npos) {
    const long long nblk = em_blocks(npos, EM_RUN);
    return nblk < EMG_MAXBLOCKS ? nblk : EMG_MAXBLOCKS;
}
static long long emgw_max_blocks(int rows, int s) {
    const long long fit = (long long)(EMGW_PART_BYTES / ((size_t)rows * s * sizeof(float)));
    return fit < EMG_MAXBLOCKS ? fit : EMG_MAXBLOCKS;
}

// dynamic LDS of the backwards: the tables, 8 stages of 16 x max(16 nt + 4, s + 5) floats, dBexp [states][16 kt]
static size_t emg_lds_bytes(int nc, int s, int nt, int kt, int states) {
    const int qs = 16 * nt + 4, w = s + 5;
    return ((size_t)2 * (nc > 0 ? nc : 1) * 512 + (size_t)(EM_THREADS / 64) * 16 * (qs > w ? qs : w) +
            (size_t)states * 16 * kt) * sizeof(float);
}

extern "C" size_t hmm_gene_emissions_grad_workspace_bytes(int b, int L, int s, int rows, int q) {
    if (b < 1 || L < 1 || s < 1 || rows < 1 || q < 1) return 0;
    if (q > EM_MAXQ || s > EM_MAXS || rows > EM_MAXR) return 0;
    const size_t bytes = (size_t)emg_blocks((long long)b * L) * rows * s * sizeof(float);
    return (bytes + 255) & ~(size_t)255;
}

extern "C" size_t hmm_gene_emissions_grad_wide_workspace_bytes(int b, int L, int s, int rows, int q) {
    if (b < 1 || L < 1 || s < 1 || rows < 1 || q < 1) return 0;
    if (q > EMW_MAXQ || s > EM_MAXS || rows > EMW_MAXR) return 0;
    const size_t bytes = (size_t)emgw_max_blocks(rows, s) * rows * s * sizeof(float);
    return (bytes + 255) & ~(size_t)255;
}

// the checks every backward entry point makes, in the documented order; need = its workspace query's answer
static int emg_check_args(int b, int L, int s, int q, int rows, int nc, int maxq, int maxr, const void *x, const void *B,
                          const void *state_row, const void *codon, const void *state_codon, const void *dE,
                          const void *dx, const void *dB, const void *workspace, size_t workspace_bytes, size_t need) {
    if (int err = em_check_args(b, L, s, q, rows, nc, maxq, maxr, x, B, state_row, codon, state_codon,
                                dE && (dx || dB) && workspace))
        return err;
    return workspace_bytes < need || ((uintptr_t)workspace & 255) ? HMM_ERR_WORKSPACE : HMM_OK;
}

extern "C" int hmm_gene_emissions_grad(const float *x, int b, int L, int s, const float *B, int rows,
                                       const int *state_row, const float *codon, int nc, const int *state_codon, int q,
                                       float free_value, float add, int n_mass, const float *dE, float *dx, float *dB,
                                       void *workspace, size_t workspace_bytes, void *stream) {
    if (int err = emg_check_args(b, L, s, q, rows, nc, EM_MAXQ, EM_MAXR, x, B, state_row, codon, state_codon, dE, dx, dB,
                                 workspace, workspace_bytes, hmm_gene_emissions_grad_workspace_bytes(b, L, s, rows, q)))
        return err;
    const long long npos = (long long)b * L;
    const int nblk = (int)emg_blocks(npos);
    const bool small = q <= 16 && s <= 16;
    const size_t lds = small ? emg_lds_bytes(nc, s, 1, 1, 16) : emg_lds_bytes(nc, s, 4, 2, 64);
    float *part = dB ? (float *)workspace : nullptr;
    hipStream_t st = (hipStream_t)stream;
#define EMG_LAUNCH(NT_, KT_)                                                                                              \
    hipLaunchKernelGGL((k_gene_emissions_grad<NT_, KT_>), dim3((unsigned)nblk), dim3(EM_THREADS), lds, st, x, npos, L, s, B, \
                       state_row, codon, nc, state_codon, q, rows, free_value, add, (float)n_mass, dE, dx, part)
    if (small) EMG_LAUNCH(1, 1);
    else EMG_LAUNCH(4, 2);
#undef EMG_LAUNCH
    if (dB)
        hipLaunchKernelGGL(k_gene_emissions_grad_sum, dim3((unsigned)((rows * s + 63) / 64)), dim3(64), 0, st, part, nblk,
                           rows * s, dB);
    return check_launch();
}

extern "C" int hmm_gene_emissions_grad_wide(const float *x, int b, int L, int s, const float *B, int rows,
                                            const int *state_row, const float *codon, int nc, const int *state_codon, int q,
                                            float free_value, float add, int n_mass, const float *dE, float *dx, float *dB,
                                            void *workspace, size_t workspace_bytes, void *stream) {
    if (int err = emg_check_args(b, L, s, q, rows, nc, EMW_MAXQ, EMW_MAXR, x, B, state_row, codon, state_codon, dE, dx, dB,
                                 workspace, workspace_bytes, hmm_gene_emissions_grad_wide_workspace_bytes(b, L, s, rows, q)))
        return err;
    const long long npos = (long long)b * L;
    const int run_len = emw_run_len(npos);
    const long long cap = emgw_max_blocks(rows, s), want = em_blocks(npos, run_len);
    const int nblk = (int)(want < cap ? want : cap);
    float *part = dB ? (float *)workspace : nullptr;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_gene_emissions_grad_wide, dim3((unsigned)nblk), dim3(EM_THREADS),
                       emg_lds_bytes(nc, s, 4, 2, 64 * ((q + 63) / 64)), st, x, npos, L, s, B, state_row, codon, nc,
                       state_codon, q, rows, free_value, add, (float)n_mass, run_len, dE, dx, part);
    if (dB)
        hipLaunchKernelGGL(k_gene_emissions_grad_sum, dim3((unsigned)((rows * s + 63) / 64)), dim3(64), 0, st, part, nblk,
                           rows * s, dB);
    return check_launch();
}
