// hmm_emitter_grad.inc — backward of the fused gene emitter (hmm_emitter.inc), included by
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
// Shape of the kernel: the forward's.  A wave owns runs of EM_RUN positions and walks 16-position tiles.
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
//   2. states are folded into kernel rows in ascending state order (state_row);
//   3. the block writes its (rows, s) partial into the workspace;
//   4. k_gene_emissions_grad_sum adds the block partials in block order in fp64 and writes fp32 dB.
// dB is written whole by the call: the caller does not zero it.
//
// Compiler figures (gfx950, hipcc -O3), <NT, KT>; tables = 2 max(nc,1) x 2 KiB (36 KiB for the gene model's nc = 9):
//   <1, 1>  (q <= 16, s <= 16)   128 VGPRs, 8 B scratch (one register, stored before and reloaded once per run, outside
//                                the tile loop), LDS per block = tables + 8 stages of 1344 B + 1 KiB  (48 640 B)
//   <4, 2>  (everything else)    250 VGPRs, no scratch, LDS per block = tables + 8 stages of 4352 B + 8 KiB  (79 872 B)

#define EMG_MAXBLOCKS 1024  // block partials the second kernel sums

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
    extern __shared__ __attribute__((aligned(16))) float T9[];     // [2][max(nc,1)][512], the stages, dBexp
    constexpr int QS = 16 * NT + 4;                                // row stride of the H stage
    const int tid = threadIdx.x;
    const int w = s + 5;
    const int ncp = nc > 0 ? nc : 1;
    const int stf = 16 * (QS > w ? QS : w);                        // floats per stage
    float *stage = T9 + (size_t)2 * ncp * 512 + (size_t)(tid >> 6) * stf;
    float *red = T9 + (size_t)2 * ncp * 512 + (size_t)(EM_THREADS / 64) * stf;      // [16 NT][16 KT]
    em_build_tables(T9, codon, nc, n_mass, tid);
    for (int e = tid; e < 256 * NT * KT; e += EM_THREADS) red[e] = 0.f;
    __syncthreads();

    const int lane = tid & 63, g = lane >> 4, n = lane & 15;
    // B-operand registers of the dx product: Bexp[state 16 nt + 4g + kk][class 16 kt + n]; this lane's table rows
    f4 bx[NT][KT];
    int cj[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        cj[nt] = 16 * nt + n < q ? state_codon[16 * nt + n] : -1;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            const int j = 16 * nt + 4 * g + kk;
            const int brow = j < q ? state_row[j] : 0;
#pragma unroll
            for (int kt = 0; kt < KT; ++kt) {
                const int cls = 16 * kt + n;
                bx[nt][kt][kk] = (j < q && cls < s) ? B[brow * s + cls] : 0.f;
            }
        }
    }
    const f4 zero4 = {0.f, 0.f, 0.f, 0.f};
    f4 acc[NT][KT];                                         // dBexp[state 16 nt + 4g + r][class 16 kt + n]
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int kt = 0; kt < KT; ++kt) acc[nt][kt] = zero4;
    const int npieces = 4 * w;                              // 16-byte pieces per dx tile
    const bool want_dx = dx != nullptr, want_dB = part != nullptr;

    struct GT { f4 v[NT]; };

    const long long nruns = (npos + EM_RUN - 1) / EM_RUN;
    const long long wave0 = (long long)blockIdx.x * (EM_THREADS / 64) + (tid >> 6);
    const long long nwaves = (long long)gridDim.x * (EM_THREADS / 64);
    for (long long run = wave0; run < nruns; run += nwaves) {
        const long long P0 = run * EM_RUN;
        const long long left = npos - P0;
        const int ntiles = (int)((left < EM_RUN ? left : EM_RUN) + 15) / 16;
        int tb = (int)(P0 % L);                             // position of the tile's first row in its sequence
        // nucleotide rows are addressed relative to the run with 32-bit offsets, clamped into the tensor
        const float *xrun = x + P0 * w;
        const int omin = (int)(-(P0 < 16 ? P0 : 16) * w);
        const int omax = (int)((left - 1 < EM_RUN + 48 ? left - 1 : EM_RUN + 48) * w);

        auto load_nuc = [&](int rel) {                      // nucleotides of position n of the tile at P0 + rel
            int off = (rel + n) * w;
            off = off < omin ? omin : (off > omax ? omax : off);
            return em_load_nuc(xrun + off, s);
        };
        auto load_G = [&](long long Pt) {                   // the dE tile at Pt in the D layout, 0 outside
            GT gt;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const long long pos = Pt + 4 * g + r;
                    const int j = 16 * nt + n;
                    gt.v[nt][r] = (pos < npos && j < q) ? dE[pos * q + j] : 0.f;
                }
            return gt;
        };

        EmCodes prev = em_classify(load_nuc(-16), n);       // codes only (clamped at the tensor start)
        EmCodes cur = em_classify(load_nuc(0), n);
        EmNuc ra = load_nuc(16);
        GT gcur = load_G(P0);
        for (int i = 0; i < ntiles; ++i) {
            const int rel = 16 * i;
            const long long P = P0 + rel;
            const EmNuc rb = load_nuc(rel + 32);            // two tiles ahead
            const GT gnx = load_G(P + 16);                  // one tile ahead
            f4 xb[KT];                                      // B operand of the dB product: x[P + 4g + r][16 kt + n]
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
            const EmCodes nxt = em_classify(ra, n);
            em_scale_tile<NT>(gcur.v, stage, QS, cj, q, T9, ncp, prev, cur, nxt, tb, L, P, npos, g, n, x, s, w, free_value,
                              add, n_mass);
            __builtin_amdgcn_wave_barrier();                // stage is wave-private: LDS ops of a wave execute in order
            f4 Hd[NT], Ha[NT];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                Ha[nt] = *reinterpret_cast<const f4 *>(stage + n * QS + 16 * nt + 4 * g);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float v = stage[(4 * g + r) * QS + 16 * nt + n];
                    Hd[nt][r] = (P + 4 * g + r < npos && 16 * nt + n < q) ? v : 0.f;
                    Ha[nt][r] = (P + n < npos && 16 * nt + 4 * g + r < q) ? Ha[nt][r] : 0.f;
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
                    f4 Dx = zero4;                          // dx[P + 4g + r][class 16 kt + n]
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
                {   // flush the tile: 64 (s + 5) contiguous bytes of dx, 16 bytes per lane
                    const long long nfl = (npos - P < 16 ? npos - P : 16) * w;      // floats that exist
                    float *dst = dx + P * w;
                    for (int pc = lane; pc < npieces; pc += 64) {
                        if (4 * pc + 3 < nfl) {
                            *reinterpret_cast<f4 *>(dst + 4 * pc) = *reinterpret_cast<const f4 *>(stage + 4 * pc);
                        } else {
                            for (int u2 = 4 * pc; u2 < nfl; ++u2) dst[u2] = stage[u2];
                        }
                    }
                }
                __builtin_amdgcn_wave_barrier();
            }
            prev = cur; cur = nxt;
            ra = rb;
            gcur = gnx;
            tb += 16;
            if (tb >= L) tb %= L;
        }
    }

    if (want_dB) {
        // waves in fixed order into one copy of dBexp, then states into rows in ascending state order
        for (int wv = 0; wv < EM_THREADS / 64; ++wv) {
            if ((tid >> 6) == wv) {
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                    for (int kt = 0; kt < KT; ++kt)
#pragma unroll
                        for (int r = 0; r < 4; ++r) red[(16 * nt + 4 * g + r) * (16 * KT) + 16 * kt + n] += acc[nt][kt][r];
            }
            __syncthreads();
        }
        float *dst = part + (size_t)blockIdx.x * rows * s;
        for (int e = tid; e < rows * s; e += EM_THREADS) {
            const int rr = e / s, c = e - rr * s;
            float sum = 0.f;
            for (int j = 0; j < q; ++j)
                if (state_row[j] == rr) sum += red[j * (16 * KT) + c];
            dst[e] = sum;
        }
    }
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

static long long emg_blocks(long long npos) {
    const int wpb = EM_THREADS / 64;
    const long long nblk = ((npos + EM_RUN - 1) / EM_RUN + wpb - 1) / wpb;
    return nblk < EMG_MAXBLOCKS ? nblk : EMG_MAXBLOCKS;
}

extern "C" size_t hmm_gene_emissions_grad_workspace_bytes(int b, int L, int s, int rows, int q) {
    if (b < 1 || L < 1 || s < 1 || rows < 1 || q < 1) return 0;
    if (q > EM_MAXQ || s > EM_MAXS || rows > EM_MAXR) return 0;
    const size_t bytes = (size_t)emg_blocks((long long)b * L) * rows * s * sizeof(float);
    return (bytes + 255) & ~(size_t)255;
}

extern "C" int hmm_gene_emissions_grad(const float *x, int b, int L, int s, const float *B, int rows,
                                       const int *state_row, const float *codon, int nc, const int *state_codon, int q,
                                       float free_value, float add, int n_mass, const float *dE, float *dx, float *dB,
                                       void *workspace, size_t workspace_bytes, void *stream) {
    if (b < 1 || L < 1 || s < 1 || q < 1 || rows < 1 || nc < 0) return HMM_ERR_BAD_SHAPE;
    if (q > EM_MAXQ || s > EM_MAXS || rows > EM_MAXR || nc > EM_MAXC) return HMM_ERR_Q_UNSUPPORTED;
    if (!x || !B || !state_row || !state_codon || !dE || (nc > 0 && !codon) || (!dx && !dB) || !workspace)
        return HMM_ERR_NULL_POINTER;
    if (workspace_bytes < hmm_gene_emissions_grad_workspace_bytes(b, L, s, rows, q) || ((uintptr_t)workspace & 255))
        return HMM_ERR_WORKSPACE;
    const long long npos = (long long)b * L;
    const int nblk = (int)emg_blocks(npos);
    const bool small = q <= 16 && s <= 16;
    const int qs = 16 * (small ? 1 : 4) + 4, w = s + 5;
    const size_t lds = ((size_t)2 * (nc > 0 ? nc : 1) * 512 + (size_t)(EM_THREADS / 64) * 16 * (qs > w ? qs : w) +
                        (small ? 256 : 256 * 4 * 2)) * sizeof(float);
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
