// hmm_emitter_mvn_grad_wide.inc — backward of the embedding-emission factor for up to 256 states and 256 kernel
// rows.  Included by hmm_engine.hip after hmm_emitter_mvn_wide.inc and hmm_emitter_mvn_grad.inc.  Arguments, layouts
// and formulas are those of hmm_embedding_emissions_grad (hmm_emitter_mvn_grad.inc), all in the difference form:
//
//   g[p][r]  = exp(inv_temperature * (log_norm[r] - 0.5 md[p][r])),   f = g + add
//   dE_in[p][j]   = dE[p][j] * f[p][row(j)]
//   Gf[p][r]      = sum_{j: row(j) = r} dE[p][j] * E_in[p][j]          (ascending j)
//   W[p][r]       = inv_temperature * Gf[p][r] * g[p][r]
//   dlog_norm[r]  = sum_p W[p][r]
//   dmean[r][c]   = inv_std[r][c]^2 * sum_p W[p][r] * (x[p][c] - mean[r][c])
//   dinv_std[r][c] = -inv_std[r][c] * sum_p W[p][r] * (x[p][c] - mean[r][c])^2
//   demb[p][c]    = -sum_r W[p][r] * (x[p][c] - mean[r][c]) * inv_std[r][c]^2
//
// None of the 64-state layouts stretches to 256 rows (a 256 x (q | 1) stage of dE * E_in, three accumulators per
// row in registers).  Four kernels:
//   k_embedding_emissions_grad_w_wide   lane = position; work item = (tile of 256 positions, block of 32 rows), as
//        the wide forward (mv_md gives md, then g, of the block's rows in LDS).  The block's states — a contiguous
//        piece of the row-sorted state list — are taken 32 at a time: lane (position e / 32, entry e % 32) reads dE
//        (and E_in), writes dE_in and parks dE * E_in in LDS (row stride 33; the slice stage is free by then);
//        then lane p adds its position's entries in list order, that is row by row and in ascending state order
//        within a row, carrying the open row's sum over chunk borders, and turns g[r][p] into W[p][r] in place when
//        a row closes (a row without states closes with Gf = 0).  At the end the block's W leaves flat, 32 rows
//        (128 bytes) per position, padding rows up to RS = rows rounded up to 4 as 0.
//   k_embedding_emissions_grad_x_wide   lane = column, demb alone: cw columns (the power of two >= d, at most 256;
//        blockIdx.y picks the 256-column chunk) x 256 / cw position groups; four positions per lane at a time, the
//        rows in ascending order in the inner loop (mean / inv_std of the lane's column through L1, W[p][.]
//        wave-uniform for cw >= 64).  demb[p][c] = -(sum over r = 0 .. rows - 1, one fma each).
//   k_embedding_emissions_grad_tab_wide lane = column, the table sums of one block of 32 rows (blockIdx.z): mean of
//        the lane's column and the three accumulators per row in registers, as the 64-state table kernel with RB =
//        32 but without demb.  Workgroup x walks tiles x, x + gridDim.x, ... in order, positions of a tile in
//        order; at the end the position groups are added in group order through LDS, one partial per workgroup.
//   k_embedding_emissions_grad_sum      (hmm_emitter_mvn_grad.inc, unchanged) adds the partials in workgroup order
//        in fp64 and applies inv_std^2 / -inv_std.
// No atomics.  Every order above is fixed by (b L, d, rows, q) and the row map alone: repeated calls and calls for
// any subset of the outputs are bit-identical (each kernel computes the same values whatever is stored).
//
// Workspace: W, b L x RS floats, then at most MVG_MAXBLOCKS partials of rows (2 d + 1) floats, held under
// MVG_PART_BYTES (16 MiB) by shrinking the table kernel's x extent as rows * d grows.
//
// Compiler figures (gfx950, hipcc -O3): see DESIGN §10e.

#define MVGW_HS (MVW_SC + 1)          // LDS row stride of the parked dE * E_in chunk
#define MVGW_STAGE (MV_THREADS * (MV_XS > MVGW_HS ? MV_XS : MVGW_HS))

__global__ __launch_bounds__(MV_THREADS) void k_embedding_emissions_grad_w_wide(
    const float *__restrict__ emb, long long ld, long long npos, int d, const float *__restrict__ mean,
    const float *__restrict__ inv_std, const float *__restrict__ log_norm, int rows, const int *__restrict__ state_row,
    int q, float inv_temperature, float add, const float *__restrict__ E_in, const float *__restrict__ dE,
    float *__restrict__ dE_in, float *__restrict__ W, int RS) {
    extern __shared__ __attribute__((aligned(16))) float mv_lds[];
    float *xs = mv_lds;                                   // [MV_THREADS][MV_XS], then hs [MV_THREADS][MVGW_HS]
    float *hs = mv_lds;
    float *fs = xs + MVGW_STAGE;                          // [MVW_RB][MV_FS]: md, then g, then W, of the item's rows
    int *srow = reinterpret_cast<int *>(fs + MVW_RB * MV_FS);   // [q]
    int *rstart = srow + q;                               // [rows + 1]
    int *rlist = rstart + rows + 1;                       // [q]
    const int tid = threadIdx.x;
    const int nrb = (rows + MVW_RB - 1) / MVW_RB;
    const long long ntiles = (npos + MV_THREADS - 1) / MV_THREADS;
    const long long nitems = ntiles * nrb;
    long long item = blockIdx.x;
    if (item >= nitems) return;
    mv_row_lists(state_row, q, rows, srow, rstart, rlist, tid);

    MvSlice pre = mv_load(emb, ld, npos, d, (item / nrb) * MV_THREADS, 0, tid);
    for (; item < nitems; item += gridDim.x) {
        const long long P0 = (item / nrb) * MV_THREADS;
        const int r0 = (int)(item % nrb) * MVW_RB;
        const int nr = rows - r0 < MVW_RB ? rows - r0 : MVW_RB;
        const long long nxt = item + gridDim.x;
        mv_md(emb, ld, npos, d, mean, inv_std, r0, nr, P0, nxt < nitems ? (nxt / nrb) * MV_THREADS : -1, pre, xs, fs, tid);
        // md -> g, in place
#pragma unroll 1
        for (int r = 0; r < nr; ++r)
            fs[r * MV_FS + tid] = expf(inv_temperature * (log_norm[r0 + r] - 0.5f * fs[r * MV_FS + tid]));
        const int kend = rstart[r0 + nr];
        const int kk = tid & (MVW_SC - 1);
        int rcur = r0;                                    // the open row (workgroup-uniform) and its sum so far
        float gf = 0.f;
        for (int kc = rstart[r0]; kc < kend; kc += MVW_SC) {
            __syncthreads();                              // g complete and the slice stage free / the previous chunk folded
            if (kc + kk < kend) {
                const int j = rlist[kc + kk];
                const float *grow = fs + (srow[j] - r0) * MV_FS;
                for (int p = tid / MVW_SC; p < MV_THREADS; p += MV_THREADS / MVW_SC) {
                    const long long pos = P0 + p;
                    if (pos >= npos) break;
                    const long long at = pos * q + j;
                    const float gv = dE[at];
                    if (dE_in) dE_in[at] = gv * (grow[p] + add);
                    if (W) hs[p * MVGW_HS + kk] = E_in ? gv * E_in[at] : gv;
                }
            }
            if (!W) continue;
            __syncthreads();
            const int kstop = kc + MVW_SC < kend ? kc + MVW_SC : kend;
            if (P0 + tid < npos) {
                const float *hrow = hs + tid * MVGW_HS - kc;
                for (int k = kc; k < kstop; ++k) {
                    while (rstart[rcur + 1] <= k) {       // rows that ended before entry k
                        fs[(rcur - r0) * MV_FS + tid] = inv_temperature * gf * fs[(rcur - r0) * MV_FS + tid];
                        gf = 0.f;
                        ++rcur;
                    }
                    gf += hrow[k];
                }
            }
        }
        if (!W) continue;
        for (; rcur < r0 + nr; ++rcur) {                  // the open row and the rows after it (no states: Gf = 0)
            fs[(rcur - r0) * MV_FS + tid] = inv_temperature * gf * fs[(rcur - r0) * MV_FS + tid];
            gf = 0.f;
        }
        __syncthreads();
        // W[p][r0 .. r0 + 32) out, rows from `rows` up to RS as 0
        const int nw = RS - r0 < MVW_RB ? RS - r0 : MVW_RB;
        if (kk < nw) {
            for (int p = tid / MVW_RB; p < MV_THREADS; p += MV_THREADS / MVW_RB) {
                const long long pos = P0 + p;
                if (pos >= npos) break;
                W[pos * RS + r0 + kk] = kk < nr ? fs[kk * MV_FS + p] : 0.f;
            }
        }
    }
}

// demb alone.  WIDE: cw >= 64, so a wave shares its position group and W[p][.] is wave-uniform.
template <bool WIDE>
__global__ __launch_bounds__(MV_THREADS) void k_embedding_emissions_grad_x_wide(
    const float *__restrict__ emb, long long ld, long long npos, int d, const float *__restrict__ mean,
    const float *__restrict__ inv_std, int rows, const float *__restrict__ W, int RS, int cshift,
    float *__restrict__ demb, long long ldd) {
    const int tid = threadIdx.x;
    const int cw = 1 << cshift, npg = MV_THREADS >> cshift;
    const int c = tid & (cw - 1);
    int pg = tid >> cshift;
    if (WIDE) pg = __builtin_amdgcn_readfirstlane(pg);
    const int col = blockIdx.y * MVG_CW + c;
    if (col >= d) return;                                 // no barrier below
    const float *mcol = mean + col, *scol = inv_std + col;
    const long long ntiles = (npos + MV_THREADS - 1) / MV_THREADS;
    for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long long P0 = tile * MV_THREADS;
        for (int i0 = 0; i0 < cw; i0 += 4) {
            float xv[4], de[4];
            const float *wp[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                long long pos = P0 + (long long)(i0 + u) * npg + pg;
                if (i0 + u >= cw || pos >= npos) pos = P0;      // computed, not stored; P0 < npos
                xv[u] = emb[pos * ld + col];
                wp[u] = W + pos * RS;
                de[u] = 0.f;
            }
            for (int r4 = 0; r4 < rows; r4 += 4) {
                f4 w4[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) w4[u] = *reinterpret_cast<const f4 *>(wp[u] + r4);
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    if (r4 + v < rows) {
                        const float m = mcol[(size_t)(r4 + v) * d], s = scol[(size_t)(r4 + v) * d];
                        const float iv = s * s;
#pragma unroll
                        for (int u = 0; u < 4; ++u) de[u] = fmaf(w4[u][v] * (xv[u] - m), iv, de[u]);
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const long long pos = P0 + (long long)(i0 + u) * npg + pg;
                if (i0 + u < cw && pos < npos) demb[pos * ldd + col] = -de[u];
            }
        }
    }
}

// the table sums of rows [32 blockIdx.z, 32 blockIdx.z + 32)
template <bool WIDE>
__global__ __launch_bounds__(MV_THREADS) void k_embedding_emissions_grad_tab_wide(
    const float *__restrict__ emb, long long ld, long long npos, int d, const float *__restrict__ mean, int rows,
    const float *__restrict__ W, int RS, int cshift, float *__restrict__ part) {
    __shared__ float red[MV_THREADS];
    const int tid = threadIdx.x;
    const int cw = 1 << cshift, npg = MV_THREADS >> cshift;
    const int c = tid & (cw - 1);
    int pg = tid >> cshift;
    if (WIDE) pg = __builtin_amdgcn_readfirstlane(pg);
    const int col = blockIdx.y * MVG_CW + c;
    const bool active = col < d;
    const int r0 = blockIdx.z * MVW_RB;
    const int nr = rows - r0 < MVW_RB ? rows - r0 : MVW_RB;
    float m[MVW_RB], am[MVW_RB], as[MVW_RB], aw[MVW_RB];
#pragma unroll
    for (int r = 0; r < MVW_RB; ++r) {
        m[r] = active && r < nr ? mean[(size_t)(r0 + r) * d + col] : 0.f;
        am[r] = as[r] = aw[r] = 0.f;
    }
    const long long ntiles = (npos + MV_THREADS - 1) / MV_THREADS;
    for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long long P0 = tile * MV_THREADS;
        for (int i0 = 0; i0 < cw; i0 += 4) {
            float xv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {                 // four positions' loads in flight
                const long long pos = P0 + (long long)(i0 + u) * npg + pg;
                xv[u] = (i0 + u < cw && pos < npos && active) ? emb[pos * ld + col] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const long long pos = P0 + (long long)(i0 + u) * npg + pg;
                if (i0 + u < cw && pos < npos) {
                    const float *wp = W + pos * RS + r0;
                    const float x = xv[u];
#pragma unroll
                    for (int r4 = 0; r4 < MVW_RB; r4 += 4) {
                        if (r4 < nr) {
                            const f4 w4 = *reinterpret_cast<const f4 *>(wp + r4);
#pragma unroll
                            for (int v = 0; v < 4; ++v) {
                                const int r = r4 + v;
                                const float t = x - m[r];
                                const float wt = w4[v] * t;
                                am[r] += wt;
                                as[r] = fmaf(wt, t, as[r]);
                                aw[r] += w4[v];
                            }
                        }
                    }
                }
            }
        }
    }
    // position groups in group order, one partial per workgroup: [rows][d] sum W t, [rows][d] sum W t^2, [rows] sum W
    const int nel = rows * (2 * d + 1);
    float *dst = part + (size_t)blockIdx.x * nel;
#pragma unroll
    for (int r = 0; r < MVW_RB; ++r) {
        if (r < nr) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                __syncthreads();
                red[tid] = k == 0 ? am[r] : (k == 1 ? as[r] : aw[r]);
                __syncthreads();
                if (pg == 0 && (k < 2 ? active : (tid == 0 && blockIdx.y == 0))) {
                    float sum = red[c];
                    for (int g = 1; g < npg; ++g) sum += red[g * cw + c];
                    if (k < 2) dst[(size_t)(k * rows + r0 + r) * d + col] = sum;
                    else dst[(size_t)2 * rows * d + r0 + r] = sum;
                }
            }
        }
    }
}

static bool mvgw_supported(int b, int L, int d, int rows, int q) {
    return b >= 1 && L >= 1 && d >= 1 && rows >= 1 && q >= 1 && q <= MVW_MAXQ && rows <= MVW_MAXR && d <= MVG_MAXD;
}

// W (b L x rows rounded up to 4 floats), then the partials: min(tiles, 1024) of rows (2 d + 1) floats, at most 16 MiB
extern "C" size_t hmm_embedding_emissions_grad_wide_workspace_bytes(int b, int L, int d, int rows, int q) {
    if (!mvgw_supported(b, L, d, rows, q)) return 0;
    const long long npos = (long long)b * L;
    const size_t parts = (size_t)mvg_blocks(npos, d, rows) * rows * (2 * (size_t)d + 1) * sizeof(float);
    return mvg_w_bytes(npos, rows) + ((parts + 255) & ~(size_t)255);
}

extern "C" int hmm_embedding_emissions_grad_wide(const float *emb, long long ld, int b, int L, int d, const float *mean,
                                                 const float *inv_std, const float *log_norm, int rows,
                                                 const int *state_row, int q, float inv_temperature, float add,
                                                 const float *E_in, const float *dE, float *dE_in, float *demb,
                                                 long long ldd, float *dmean, float *dinv_std, float *dlog_norm,
                                                 void *workspace, size_t workspace_bytes, void *stream) {
    if (b < 1 || L < 1 || d < 1 || rows < 1 || q < 1 || ld < d || (demb && ldd < d)) return HMM_ERR_BAD_SHAPE;
    if (q > MVW_MAXQ || rows > MVW_MAXR || d > MVG_MAXD) return HMM_ERR_Q_UNSUPPORTED;
    const int ntab = (dmean != nullptr) + (dinv_std != nullptr) + (dlog_norm != nullptr);
    if (!emb || !mean || !inv_std || !log_norm || !state_row || !dE || !workspace) return HMM_ERR_NULL_POINTER;
    if ((!dE_in && !demb && ntab == 0) || (ntab != 0 && ntab != 3) || (dE_in && !E_in)) return HMM_ERR_NULL_POINTER;
    if (workspace_bytes < hmm_embedding_emissions_grad_wide_workspace_bytes(b, L, d, rows, q) ||
        ((uintptr_t)workspace & 255))
        return HMM_ERR_WORKSPACE;
    const long long npos = (long long)b * L;
    const long long ntiles = (npos + MV_THREADS - 1) / MV_THREADS;
    const int RS = (rows + 3) & ~3;
    const bool second = demb || ntab;
    float *W = second ? (float *)workspace : nullptr;
    float *part = (float *)((char *)workspace + mvg_w_bytes(npos, rows));
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_embedding_emissions_grad_w_wide, dim3(mvw_grid(npos, rows)), dim3(MV_THREADS),
                       mvw_lds_bytes(MVGW_STAGE, rows, q), st, emb, ld, npos, d, mean, inv_std, log_norm, rows, state_row,
                       q, inv_temperature, add, E_in, dE, dE_in, W, RS);
    if (second) {
        int cshift = 0;
        while ((1 << cshift) < d && cshift < 8) ++cshift;
        const unsigned ny = (unsigned)((d + MVG_CW - 1) / MVG_CW);
        if (demb) {
            const dim3 grid((unsigned)(ntiles < MVW_MAXGRID ? ntiles : MVW_MAXGRID), ny);
            if (cshift >= 6)
                hipLaunchKernelGGL((k_embedding_emissions_grad_x_wide<true>), grid, dim3(MV_THREADS), 0, st, emb, ld, npos, d,
                                   mean, inv_std, rows, W, RS, cshift, demb, ldd);
            else
                hipLaunchKernelGGL((k_embedding_emissions_grad_x_wide<false>), grid, dim3(MV_THREADS), 0, st, emb, ld, npos, d,
                                   mean, inv_std, rows, W, RS, cshift, demb, ldd);
        }
        if (ntab) {
            const int nblk = mvg_blocks(npos, d, rows);
            const dim3 grid((unsigned)nblk, ny, (unsigned)((rows + MVW_RB - 1) / MVW_RB));
            if (cshift >= 6)
                hipLaunchKernelGGL((k_embedding_emissions_grad_tab_wide<true>), grid, dim3(MV_THREADS), 0, st, emb, ld, npos, d,
                                   mean, rows, W, RS, cshift, part);
            else
                hipLaunchKernelGGL((k_embedding_emissions_grad_tab_wide<false>), grid, dim3(MV_THREADS), 0, st, emb, ld, npos, d,
                                   mean, rows, W, RS, cshift, part);
            hipLaunchKernelGGL(k_embedding_emissions_grad_sum, dim3((unsigned)((rows * (2 * d + 1) + 63) / 64)), dim3(64), 0,
                               st, part, nblk, rows, d, inv_std, dmean, dinv_std, dlog_norm);
        }
    }
    return check_launch();
}
