// hmm_emitter_mvn_grad.inc — backward of the embedding-emission factor (hmm_emitter_mvn.inc), included by
// hmm_engine.hip after it.  Replaces autograd through SimpleGenePredHMMEmitter.embedding_log_pdf / exp / the
// product with E, which keeps a (b L, rows, d) difference tensor, its square and its product alive until
// backward().  With the forward's
//
//   md[p][r] = sum_c ((x[p][c] - mean[r][c]) * inv_std[r][c])^2
//   g[p][r]  = exp(inv_temperature * (log_norm[r] - 0.5 md[p][r])),   f = g + add
//   E_out[p][j] = E_in[p][j] * f[p][row(j)]      (multiply; without it E_in = 1)
//
// and dE = dL/dE_out:
//
//   dE_in[p][j]   = dE[p][j] * f[p][row(j)]
//   Gf[p][r]      = sum_{j: row(j) = r} dE[p][j] * E_in[p][j]          (ascending j)
//   W[p][r]       = inv_temperature * Gf[p][r] * g[p][r]               (g, not f: add carries no gradient)
//   dlog_norm[r]  = sum_p W[p][r]
//   dmean[r][c]   = inv_std[r][c]^2 * sum_p W[p][r] * (x[p][c] - mean[r][c])
//   dinv_std[r][c] = -inv_std[r][c] * sum_p W[p][r] * (x[p][c] - mean[r][c])^2
//   demb[p][c]    = -sum_r W[p][r] * (x[p][c] - mean[r][c]) * inv_std[r][c]^2
//
// Everything is evaluated in the difference form, (x - mean) first: expanded to sum_p W x and sum_p W x^2 the
// parameter gradients are a GEMM, but they cancel exactly where the forward's expansion would (an embedding
// next to one row's far-from-zero mean, and it is that row's gradient that matters).
//
// Two kernels and a small sum, because the two halves want opposite layouts:
//   k_embedding_emissions_grad_w     lane = position.  The forward's tile walk (mv_md, unchanged) gives
//        md, then g, in LDS.  The tile of dE (and E_in) is walked flat in 16-byte pieces: dE_in leaves at once,
//        dE * E_in is parked in LDS (the slice stage is free by then; row stride q | 1).  Lane p then folds its
//        position's states into rows in ascending state order and writes W[p][0 .. RS) (RS = rows rounded up
//        to 4, the padding 0) to the workspace with 16-byte stores.
//   k_embedding_emissions_grad_tab   lane = column.  A workgroup is cw columns (the power of two >= d, at most
//        256; blockIdx.y picks the 256-column chunk of a wider d) x 256 / cw position groups.  mean and
//        inv_std^2 of the lane's column sit in registers for all rows, next to the three accumulators per row;
//        x[p][c] is read in place, coalesced along c (the second read of the embedding, from L2 for the most
//        part); W[p][.] is wave-uniform for cw >= 64 and arrives through the scalar cache.  Per (p, r, c):
//        sub, mul, add, fma, fma.  demb leaves through its own row stride, coalesced, once.  The accumulators
//        live over all the tiles of the workgroup; at the end the position groups are added in group order
//        through LDS and the workgroup writes one partial.  No LDS and no barrier inside the loop.
//   k_embedding_emissions_grad_sum   adds the workgroup partials in workgroup order in fp64, applies
//        inv_std^2 / -inv_std in fp64 and writes fp32.  The three outputs are written whole.
// No atomics; the summation order is fixed by (b L, d, rows) alone, so repeated calls and calls for a subset
// of the outputs are bit-identical (every kernel computes the same values whatever is stored).
//
// Workspace: W, b L x RS floats, then at most MVG_MAXBLOCKS partials of rows (2 d + 1) floats, held under
// MVG_PART_BYTES (16 MiB) by shrinking the grid's x extent as rows * d grows (the y extent, d / 256, grows
// instead); the partials stop growing with b L.
//
// Compiler figures (gfx950, hipcc -O3): see DESIGN §10c.

#define MVG_MAXD MV_MAXD
#define MVG_CW 256                    // columns per workgroup of the table kernel
#define MVG_MAXBLOCKS 1024            // workgroup partials the sum kernel adds
#define MVG_PART_BYTES ((size_t)16 << 20)

__global__ __launch_bounds__(MV_THREADS) void k_embedding_emissions_grad_w(
    const float *__restrict__ emb, long long ld, long long npos, int d, const float *__restrict__ mean,
    const float *__restrict__ inv_std, const float *__restrict__ log_norm, int rows, const int *__restrict__ state_row,
    int q, float inv_temperature, float add, const float *__restrict__ E_in, const float *__restrict__ dE,
    float *__restrict__ dE_in, float *__restrict__ W, int RS) {
    extern __shared__ __attribute__((aligned(16))) float mv_lds[];
    const int QS = q | 1;                                 // row stride of the parked dE * E_in tile
    float *xs = mv_lds;                                   // [MV_THREADS][MV_XS], then hs [MV_THREADS][QS]
    float *hs = mv_lds;
    float *fs = xs + MV_THREADS * (MV_XS > QS ? MV_XS : QS);    // [rows][MV_FS]: md, then g
    int *srow = reinterpret_cast<int *>(fs + rows * MV_FS);     // [q]
    int *rstart = srow + q;                               // [rows + 1]: states of row r are rlist[rstart[r] .. rstart[r + 1])
    int *rlist = rstart + rows + 1;                       // [q], ascending within a row
    const int tid = threadIdx.x;
    const long long ntiles = (npos + MV_THREADS - 1) / MV_THREADS;
    long long tile = blockIdx.x;
    if (tile >= ntiles) return;
    mv_row_lists(state_row, q, rows, srow, rstart, rlist, tid);
    const unsigned qmagic = (unsigned)((0x100000000ull + (unsigned)q - 1u) / (unsigned)q);   // as in the forward

    MvSlice pre = mv_load(emb, ld, npos, d, tile * MV_THREADS, 0, tid);
    for (; tile < ntiles; tile += gridDim.x) {
        const long long P0 = tile * MV_THREADS;
        mv_md(emb, ld, npos, d, mean, inv_std, 0, rows, P0, tile + gridDim.x < ntiles ? (tile + gridDim.x) * MV_THREADS : -1, pre,
              xs, fs, tid);
        // md -> g, in place
#pragma unroll 1
        for (int r = 0; r < rows; ++r)
            fs[r * MV_FS + tid] = expf(inv_temperature * (log_norm[r] - 0.5f * fs[r * MV_FS + tid]));
        __syncthreads();                                  // g complete; the slice stage is free for hs
        // the tile of dE (and E_in), flat: dE_in out, dE * E_in into hs
        const long long left = npos - P0;
        const int nfl = (int)(left < MV_THREADS ? left : MV_THREADS) * q;     // floats that exist, <= 2^14
        const float *gsrc = dE + P0 * q;
        const float *esrc = E_in ? E_in + P0 * q : nullptr;
        float *dst = dE_in ? dE_in + P0 * q : nullptr;
        for (int e0 = 4 * tid; e0 < nfl; e0 += 4 * MV_THREADS) {
            float f[4];
            int at[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const unsigned e = (unsigned)(e0 + u) < (unsigned)nfl ? (unsigned)(e0 + u) : (unsigned)(nfl - 1);
                const unsigned p = q == 1 ? e : __umulhi(e, qmagic);
                const unsigned j = e - p * (unsigned)q;
                f[u] = fs[srow[j] * MV_FS + p] + add;
                at[u] = (int)(p * (unsigned)QS + j);
            }
            if (e0 + 4 <= nfl) {
                const f4 gv = *reinterpret_cast<const f4u *>(gsrc + e0);
                f4 ev = {1.f, 1.f, 1.f, 1.f};
                if (esrc) ev = *reinterpret_cast<const f4u *>(esrc + e0);
                if (dst) {
                    const f4 fv = {f[0], f[1], f[2], f[3]};
                    *reinterpret_cast<f4u *>(dst + e0) = gv * fv;
                }
                if (W) {
                    const f4 hv = gv * ev;
                    hs[at[0]] = hv.x; hs[at[1]] = hv.y; hs[at[2]] = hv.z; hs[at[3]] = hv.w;
                }
            } else {
                for (int u = 0; e0 + u < nfl; ++u) {
                    const float gv = gsrc[e0 + u];
                    if (dst) dst[e0 + u] = gv * f[u];
                    if (W) hs[at[u]] = esrc ? gv * esrc[e0 + u] : gv;
                }
            }
        }
        if (W) {
            __syncthreads();
            // lane p: states into rows in ascending state order, W[p][.] out (padding rows 0)
            const float *hrow = hs + tid * QS;
            const long long pos = P0 + tid;
            for (int r4 = 0; r4 < RS; r4 += 4) {
                float w[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int r = r4 + u;
                    float v = 0.f;
                    if (r < rows) {
                        float gf = 0.f;
                        for (int k = rstart[r]; k < rstart[r + 1]; ++k) gf += hrow[rlist[k]];
                        v = inv_temperature * gf * fs[r * MV_FS + tid];
                    }
                    w[u] = v;
                }
                if (pos < npos) {
                    const f4 wv = {w[0], w[1], w[2], w[3]};
                    *reinterpret_cast<f4 *>(W + pos * RS + r4) = wv;
                }
            }
        }
    }
}

// RB: rows rounded up to 8, 16 or 32 (register arrays).  WIDE: cw >= 64, so a wave shares its position group and
// W[p][.] is wave-uniform.
template <int RB, bool WIDE>
__global__ __launch_bounds__(MV_THREADS) void k_embedding_emissions_grad_tab(
    const float *__restrict__ emb, long long ld, long long npos, int d, const float *__restrict__ mean,
    const float *__restrict__ inv_std, int rows, const float *__restrict__ W, int RS, int cshift,
    float *__restrict__ demb, long long ldd, float *__restrict__ part) {
    __shared__ float red[MV_THREADS];
    const int tid = threadIdx.x;
    const int cw = 1 << cshift, npg = MV_THREADS >> cshift;
    const int c = tid & (cw - 1);
    int pg = tid >> cshift;
    if (WIDE) pg = __builtin_amdgcn_readfirstlane(pg);
    const int col = blockIdx.y * MVG_CW + c;
    const bool active = col < d;
    float m[RB], iv[RB], am[RB], as[RB], aw[RB];
#pragma unroll
    for (int r = 0; r < RB; ++r) {
        const bool have = active && r < rows;
        const float s = have ? inv_std[(size_t)r * d + col] : 0.f;
        m[r] = have ? mean[(size_t)r * d + col] : 0.f;
        iv[r] = s * s;
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
                    const float *wp = W + pos * RS;
                    const float x = xv[u];
                    float de = 0.f;
#pragma unroll
                    for (int r4 = 0; r4 < RB; r4 += 4) {
                        if (r4 < rows) {
                            const f4 w4 = *reinterpret_cast<const f4 *>(wp + r4);
#pragma unroll
                            for (int v = 0; v < 4; ++v) {
                                const int r = r4 + v;
                                const float t = x - m[r];
                                const float wt = w4[v] * t;
                                am[r] += wt;
                                as[r] = fmaf(wt, t, as[r]);
                                aw[r] += w4[v];
                                de = fmaf(wt, iv[r], de);
                            }
                        }
                    }
                    if (demb && active) demb[pos * ldd + col] = -de;
                }
            }
        }
    }
    if (!part) return;
    // position groups in group order, one partial per workgroup: [rows][d] sum W t, [rows][d] sum W t^2, [rows] sum W
    const int nel = rows * (2 * d + 1);
    float *dst = part + (size_t)blockIdx.x * nel;
#pragma unroll
    for (int r = 0; r < RB; ++r) {
        if (r < rows) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                __syncthreads();
                red[tid] = k == 0 ? am[r] : (k == 1 ? as[r] : aw[r]);
                __syncthreads();
                if (pg == 0 && (k < 2 ? active : (tid == 0 && blockIdx.y == 0))) {
                    float sum = red[c];
                    for (int g = 1; g < npg; ++g) sum += red[g * cw + c];
                    if (k < 2) dst[(size_t)(k * rows + r) * d + col] = sum;
                    else dst[(size_t)2 * rows * d + r] = sum;
                }
            }
        }
    }
}

// the partials in workgroup order, fp64; the factors that do not depend on the position are applied here
__global__ __launch_bounds__(64) void k_embedding_emissions_grad_sum(const float *__restrict__ part, int nblk, int rows, int d,
                                                                     const float *__restrict__ inv_std,
                                                                     float *__restrict__ dmean, float *__restrict__ dinv_std,
                                                                     float *__restrict__ dlog_norm) {
    const int nel = rows * (2 * d + 1), rd = rows * d;
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (e >= nel) return;
    double sum = 0.0;
    for (int k = 0; k < nblk; ++k) sum += (double)part[(size_t)k * nel + e];
    if (e < rd) {
        const double s = (double)inv_std[e];
        dmean[e] = (float)(sum * s * s);
    } else if (e < 2 * rd) {
        dinv_std[e - rd] = (float)(-sum * (double)inv_std[e - rd]);
    } else {
        dlog_norm[e - 2 * rd] = (float)sum;
    }
}

static bool mvg_supported(int b, int L, int d, int rows, int q) {
    return b >= 1 && L >= 1 && d >= 1 && rows >= 1 && q >= 1 && q <= MV_MAXQ && rows <= MV_MAXR && d <= MVG_MAXD;
}

static size_t mvg_w_bytes(long long npos, int rows) {
    const size_t bytes = (size_t)npos * (size_t)((rows + 3) & ~3) * sizeof(float);
    return (bytes + 255) & ~(size_t)255;
}

// workgroups along x of the table kernel = partials
static int mvg_blocks(long long npos, int d, int rows) {
    const long long ntiles = (npos + MV_THREADS - 1) / MV_THREADS;
    const long long fit = (long long)(MVG_PART_BYTES / ((size_t)rows * (2 * (size_t)d + 1) * sizeof(float)));
    long long n = ntiles < MVG_MAXBLOCKS ? ntiles : MVG_MAXBLOCKS;
    if (n > fit) n = fit;
    return (int)n;
}

extern "C" int hmm_embedding_emissions_grad_max_dim(void) { return MVG_MAXD; }

// W (b L x rows rounded up to 4 floats: the design needs two kernels, W is what passes between them), then the
// partials: min(tiles, 1024) of rows (2 d + 1) floats, at most 16 MiB
extern "C" size_t hmm_embedding_emissions_grad_workspace_bytes(int b, int L, int d, int rows, int q) {
    if (!mvg_supported(b, L, d, rows, q)) return 0;
    const long long npos = (long long)b * L;
    const long long ntiles = (npos + MV_THREADS - 1) / MV_THREADS;
    size_t parts = (size_t)(ntiles < MVG_MAXBLOCKS ? ntiles : MVG_MAXBLOCKS) * rows * (2 * (size_t)d + 1) * sizeof(float);
    if (parts > MVG_PART_BYTES) parts = MVG_PART_BYTES;
    return mvg_w_bytes(npos, rows) + ((parts + 255) & ~(size_t)255);
}

extern "C" int hmm_embedding_emissions_grad(const float *emb, long long ld, int b, int L, int d, const float *mean,
                                            const float *inv_std, const float *log_norm, int rows,
                                            const int *state_row, int q, float inv_temperature, float add,
                                            const float *E_in, const float *dE, float *dE_in, float *demb, long long ldd,
                                            float *dmean, float *dinv_std, float *dlog_norm, void *workspace,
                                            size_t workspace_bytes, void *stream) {
    if (b < 1 || L < 1 || d < 1 || rows < 1 || q < 1 || ld < d || (demb && ldd < d)) return HMM_ERR_BAD_SHAPE;
    if (q > MV_MAXQ || rows > MV_MAXR || d > MVG_MAXD) return HMM_ERR_Q_UNSUPPORTED;
    const int ntab = (dmean != nullptr) + (dinv_std != nullptr) + (dlog_norm != nullptr);
    if (!emb || !mean || !inv_std || !log_norm || !state_row || !dE || !workspace) return HMM_ERR_NULL_POINTER;
    if ((!dE_in && !demb && ntab == 0) || (ntab != 0 && ntab != 3) || (dE_in && !E_in)) return HMM_ERR_NULL_POINTER;
    if (workspace_bytes < hmm_embedding_emissions_grad_workspace_bytes(b, L, d, rows, q) || ((uintptr_t)workspace & 255))
        return HMM_ERR_WORKSPACE;
    const long long npos = (long long)b * L;
    const long long ntiles = (npos + MV_THREADS - 1) / MV_THREADS;
    const int RS = (rows + 3) & ~3, QS = q | 1;
    const bool second = demb || ntab;
    float *W = second ? (float *)workspace : nullptr;
    float *part = ntab ? (float *)((char *)workspace + mvg_w_bytes(npos, rows)) : nullptr;
    hipStream_t st = (hipStream_t)stream;
    const size_t lds = ((size_t)MV_THREADS * (MV_XS > QS ? MV_XS : QS) + (size_t)rows * MV_FS) * sizeof(float) +
                       (size_t)(2 * q + rows + 1) * sizeof(int);
    hipLaunchKernelGGL(k_embedding_emissions_grad_w, dim3((unsigned)(ntiles < 256 * 16 ? ntiles : 256 * 16)),
                       dim3(MV_THREADS), lds, st, emb, ld, npos, d, mean, inv_std, log_norm, rows, state_row, q,
                       inv_temperature, add, E_in, dE, dE_in, W, RS);
    if (second) {
        int cshift = 0;
        while ((1 << cshift) < d && cshift < 8) ++cshift;
        const int nblk = mvg_blocks(npos, d, rows);
        const dim3 grid((unsigned)nblk, (unsigned)((d + MVG_CW - 1) / MVG_CW));
#define MVG_LAUNCH(RB_, WIDE_)                                                                                         \
    hipLaunchKernelGGL((k_embedding_emissions_grad_tab<RB_, WIDE_>), grid, dim3(MV_THREADS), 0, st, emb, ld, npos, d, mean, \
                       inv_std, rows, W, RS, cshift, demb, ldd, part)
        if (cshift >= 6) {
            if (rows <= 8) MVG_LAUNCH(8, true);
            else if (rows <= 16) MVG_LAUNCH(16, true);
            else MVG_LAUNCH(32, true);
        } else {
            if (rows <= 8) MVG_LAUNCH(8, false);
            else if (rows <= 16) MVG_LAUNCH(16, false);
            else MVG_LAUNCH(32, false);
        }
#undef MVG_LAUNCH
        if (ntab)
            hipLaunchKernelGGL(k_embedding_emissions_grad_sum, dim3((unsigned)((rows * (2 * d + 1) + 63) / 64)), dim3(64), 0,
                               st, part, nblk, rows, d, inv_std, dmean, dinv_std, dlog_norm);
    }
    return check_launch();
}
