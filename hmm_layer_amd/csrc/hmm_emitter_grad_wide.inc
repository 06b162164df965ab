// hmm_emitter_grad_wide.inc — backward of the wide gene emitter (hmm_emitter_wide.inc) for up to 256 states and
// 256 emission-kernel rows, included by hmm_engine.hip after hmm_emitter_grad.inc.  Same arguments and values as
// hmm_gene_emissions_grad: with H[p,j] = dE[p,j] * (cod[p,j] + add),
//
//   dx[p,c] = sum_j H[p,j] * B[state_row[j], c]   (c < s; the five nucleotide columns are exactly 0)
//   dB[r,c] = sum_p sum_{j: state_row[j] = r} H[p,j] * x[p,c]
//
// Shape of the kernel: k_gene_emissions_grad<4, 2>'s body inside a loop over groups of 64 states, the group
// OUTERMOST (group -> the wave's runs -> the run's 16-position tiles).  Per group a wave holds that group's Bexp slice
// in B-operand registers (bx[4][2]) and its 32 accumulator registers of dBexp (acc[4][2]); neither would fit for
// four groups at once.  Per tile it loads the group's 64 columns of dE in the D layout, applies em_scale_tile (H into
// the wave's stage, stride 68), reads H back in the D layout (A operand of dBexp += H^T X) and in the A layout
// (dx tile = H Bexp_g), exactly as the 64-state kernel does.
//   dx   group 0 writes the tile, every later group adds its product to what is there.  The tile leaves through the
//        stage in 16-byte pieces, piece -> lane fixed, so the same lane reads back what it wrote one group earlier:
//        plain program order of one thread, no atomics, and the sum over groups runs in ascending group order whatever
//        the grid.
//   dB   after a group's runs the waves of the workgroup add acc into rows 64 grp .. of the LDS copy of dBexp
//        (q x 32), wave 0 first.  After the last group, states are folded into kernel rows in ascending state order
//        (state_row clamped into 0..rows-1), the workgroup writes its (rows, s) partial, and
//        k_gene_emissions_grad_sum adds the partials in workgroup order in fp64 and rounds once.
// Cost of the order: x's class columns and the nucleotides are read once per group (s + 5 floats per position against
// the 64 floats of dE a group reads), and dx is read and written once more per further group.  With one run per wave
// (b L <= 8 runs x grid) a run's dx (at most 1024 (s + 5) floats) is still in L2 when the next group comes for it.
//
// Runs are emw_run_len(b L) positions long (1024, shorter where b L would leave CUs idle): a function of b L alone, so
// the summation order of dB is fixed per shape.
// The grid is min(runs / 8, 1024, 16 MiB / (rows s 4)) workgroups, so the partials stay within 16 MiB; the workspace
// is sized for that cap and does not depend on b L.
//
// LDS per workgroup: tables 2 max(nc,1) x 2 KiB + 8 stages of 16 max(68, s + 5) floats + dBexp 64 ngrp x 128 B:
// 36 864 + 34 816 + 8192 ngrp bytes for nc = 9, 104 448 B at 256 states.  One workgroup per CU.
// Compiler figures (gfx950, hipcc -O3): 250 VGPRs, no scratch (the figures of k_gene_emissions_grad<4, 2>), LDS as
// above (dynamic).

#define EMGW_PART_BYTES ((size_t)16 << 20)

__global__ __launch_bounds__(EM_THREADS, 2) void k_gene_emissions_grad_wide(const float *__restrict__ x, long long npos, int L, int s,
                                                                         const float *__restrict__ B,
                                                                         const int *__restrict__ state_row,
                                                                         const float *__restrict__ codon, int nc,
                                                                         const int *__restrict__ state_codon, int q, int rows,
                                                                         float free_value, float add, float n_mass, int run_len,
                                                                         const float *__restrict__ dE, float *dx,
                                                                         float *__restrict__ part) {
    constexpr int NT = 4, KT = 2;
    extern __shared__ __attribute__((aligned(16))) float T9[];     // [2][max(nc,1)][512], the stages, dBexp
    constexpr int QS = 16 * NT + 4;                                // row stride of the H stage
    const int tid = threadIdx.x;
    const int w = s + 5;
    const int ncp = nc > 0 ? nc : 1;
    const int ngrp = (q + 63) >> 6, qp = 64 * ngrp;
    const int stf = 16 * (QS > w ? QS : w);                        // floats per stage
    float *stage = T9 + (size_t)2 * ncp * 512 + (size_t)(tid >> 6) * stf;
    float *red = T9 + (size_t)2 * ncp * 512 + (size_t)(EM_THREADS / 64) * stf;      // [qp][16 KT]
    const bool want_dx = dx != nullptr, want_dB = part != nullptr;
    em_build_tables(T9, codon, nc, n_mass, tid);
    if (want_dB)
        for (int e = tid; e < qp * 16 * KT; e += EM_THREADS) red[e] = 0.f;
    __syncthreads();

    const int lane = tid & 63, g = lane >> 4, n = lane & 15;
    const f4 zero4 = {0.f, 0.f, 0.f, 0.f};
    const int npieces = 4 * w;                              // 16-byte pieces per dx tile
    auto row_of = [&](int j) {                              // state -> kernel row, clamped into B
        const int r = state_row[j];
        return r < 0 ? 0 : (r >= rows ? rows - 1 : r);
    };

    struct GT { f4 v[NT]; };

    const long long nruns = (npos + run_len - 1) / run_len;
    const long long wave0 = (long long)blockIdx.x * (EM_THREADS / 64) + (tid >> 6);
    const long long nwaves = (long long)gridDim.x * (EM_THREADS / 64);
#pragma unroll 1
    for (int grp = 0; grp < ngrp; ++grp) {
        const int j0 = 64 * grp, qg = q - j0;               // the group's states are j0 .. j0 + min(qg, 64) - 1
        // B-operand registers of the dx product: Bexp[state j0 + 16 nt + 4g + kk][class 16 kt + n]; this lane's table rows
        f4 bx[NT][KT];
        int cj[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            int c = 16 * nt + n < qg ? state_codon[j0 + 16 * nt + n] : -1;
            cj[nt] = c < nc ? c : nc - 1;
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                const int j = 16 * nt + 4 * g + kk;
                const int brow = j < qg ? row_of(j0 + j) : 0;
#pragma unroll
                for (int kt = 0; kt < KT; ++kt) {
                    const int cls = 16 * kt + n;
                    bx[nt][kt][kk] = (j < qg && cls < s) ? B[(size_t)brow * s + cls] : 0.f;
                }
            }
        }
        f4 acc[NT][KT];                                     // dBexp[state j0 + 16 nt + 4g + r][class 16 kt + n]
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int kt = 0; kt < KT; ++kt) acc[nt][kt] = zero4;

        for (long long run = wave0; run < nruns; run += nwaves) {
            const long long P0 = run * run_len;
            const long long left = npos - P0;
            const int ntiles = (int)((left < run_len ? left : run_len) + 15) / 16;
            int tb = (int)(P0 % L);                         // position of the tile's first row in its sequence
            // nucleotide rows are addressed relative to the run with 32-bit offsets, clamped into the tensor
            const float *xrun = x + P0 * w;
            const int omin = (int)(-(P0 < 16 ? P0 : 16) * w);
            const int omax = (int)((left - 1 < run_len + 48 ? left - 1 : run_len + 48) * w);

            auto load_nuc = [&](int rel) {                  // nucleotides of position n of the tile at P0 + rel
                int off = (rel + n) * w;
                off = off < omin ? omin : (off > omax ? omax : off);
                return em_load_nuc(xrun + off, s);
            };
            auto load_G = [&](long long Pt) {               // the group's dE tile at Pt in the D layout, 0 outside
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

            EmCodes prev = em_classify(load_nuc(-16), n);   // codes only (clamped at the tensor start)
            EmCodes cur = em_classify(load_nuc(0), n);
            EmNuc ra = load_nuc(16);
            GT gcur = load_G(P0);
            for (int i = 0; i < ntiles; ++i) {
                const int rel = 16 * i;
                const long long P = P0 + rel;
                const EmNuc rb = load_nuc(rel + 32);        // two tiles ahead
                const GT gnx = load_G(P + 16);              // one tile ahead
                f4 xb[KT];                                  // B operand of the dB product: x[P + 4g + r][16 kt + n]
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
                em_scale_tile<NT>(gcur.v, stage, QS, cj, qg, T9, ncp, prev, cur, nxt, tb, L, P, npos, g, n, x, s, w,
                                  free_value, add, n_mass);
                __builtin_amdgcn_wave_barrier();            // stage is wave-private: LDS ops of a wave execute in order
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
                        f4 Dx = zero4;                      // dx[P + 4g + r][class 16 kt + n]
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
                    {   // flush the tile: 64 (s + 5) contiguous bytes of dx, 16 bytes per lane; groups after the first
                        // add to what the same lane stored for the group before
                        const long long nfl = (npos - P < 16 ? npos - P : 16) * w;      // floats that exist
                        float *dst = dx + P * w;
                        for (int pc = lane; pc < npieces; pc += 64) {
                            if (4 * pc + 3 < nfl) {
                                f4 v = *reinterpret_cast<const f4 *>(stage + 4 * pc);
                                if (grp > 0) v += *reinterpret_cast<const f4 *>(dst + 4 * pc);
                                *reinterpret_cast<f4 *>(dst + 4 * pc) = v;
                            } else {
                                for (int u2 = 4 * pc; u2 < nfl; ++u2) dst[u2] = grp > 0 ? dst[u2] + stage[u2] : stage[u2];
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

    if (want_dB) {
        // states into rows in ascending state order
        float *dst = part + (size_t)blockIdx.x * rows * s;
        for (int e = tid; e < rows * s; e += EM_THREADS) {
            const int rr = e / s, c = e - rr * s;
            float sum = 0.f;
            for (int j = 0; j < q; ++j)
                if (row_of(j) == rr) sum += red[j * (16 * KT) + c];
            dst[e] = sum;
        }
    }
}

// workgroups: one per 8 runs, at most EMG_MAXBLOCKS and at most 16 MiB of (rows, s) partials
static long long emgw_max_blocks(int rows, int s) {
    const long long fit = (long long)(EMGW_PART_BYTES / ((size_t)rows * s * sizeof(float)));
    return fit < EMG_MAXBLOCKS ? fit : EMG_MAXBLOCKS;
}

extern "C" size_t hmm_gene_emissions_grad_wide_workspace_bytes(int b, int L, int s, int rows, int q) {
    if (b < 1 || L < 1 || s < 1 || rows < 1 || q < 1) return 0;
    if (q > EMW_MAXQ || s > EM_MAXS || rows > EMW_MAXR) return 0;
    const size_t bytes = (size_t)emgw_max_blocks(rows, s) * rows * s * sizeof(float);
    return (bytes + 255) & ~(size_t)255;
}

extern "C" int hmm_gene_emissions_grad_wide(const float *x, int b, int L, int s, const float *B, int rows,
                                            const int *state_row, const float *codon, int nc, const int *state_codon, int q,
                                            float free_value, float add, int n_mass, const float *dE, float *dx, float *dB,
                                            void *workspace, size_t workspace_bytes, void *stream) {
    if (b < 1 || L < 1 || s < 1 || q < 1 || rows < 1 || nc < 0) return HMM_ERR_BAD_SHAPE;
    if (q > EMW_MAXQ || s > EM_MAXS || rows > EMW_MAXR || nc > EM_MAXC) return HMM_ERR_Q_UNSUPPORTED;
    if (!x || !B || !state_row || !state_codon || !dE || (nc > 0 && !codon) || (!dx && !dB) || !workspace)
        return HMM_ERR_NULL_POINTER;
    if (workspace_bytes < hmm_gene_emissions_grad_wide_workspace_bytes(b, L, s, rows, q) || ((uintptr_t)workspace & 255))
        return HMM_ERR_WORKSPACE;
    const long long npos = (long long)b * L;
    const int run_len = emw_run_len(npos), wpb = EM_THREADS / 64;
    const long long cap = emgw_max_blocks(rows, s), want = ((npos + run_len - 1) / run_len + wpb - 1) / wpb;
    const int nblk = (int)(want < cap ? want : cap);
    const int qs = 16 * 4 + 4, w = s + 5, qp = 64 * ((q + 63) / 64);
    const size_t lds = ((size_t)2 * (nc > 0 ? nc : 1) * 512 + (size_t)(EM_THREADS / 64) * 16 * (qs > w ? qs : w) +
                        (size_t)qp * 32) * sizeof(float);
    float *part = dB ? (float *)workspace : nullptr;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_gene_emissions_grad_wide, dim3((unsigned)nblk), dim3(EM_THREADS), lds, st, x, npos, L, s, B,
                       state_row, codon, nc, state_codon, q, rows, free_value, add, (float)n_mass, run_len, dE, dx, part);
    if (dB)
        hipLaunchKernelGGL(k_gene_emissions_grad_sum, dim3((unsigned)((rows * s + 63) / 64)), dim3(64), 0, st, part, nblk,
                           rows * s, dB);
    return check_launch();
}
