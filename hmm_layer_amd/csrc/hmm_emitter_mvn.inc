// hmm_emitter_mvn.inc — embedding-emission factor of the gene-prediction models, included by
// hmm_engine.hip.  Replaces, for inference with one model, diagonal covariance and one mixture
// component, MvnMixture.component_log_pdf (hmm_layer/MvnMixture.py:125-149) and the exp / multiply of
// SimpleGenePredHMMEmitter.forward (hmm_layer/gene_pred_hmm_emitter.py:101-112):
//
//   md[p][r] = sum_c ((x[p][c] - mean[r][c]) * inv_std[r][c])^2
//   f[p][j]  = exp(inv_temperature * (log_norm[r] - 0.5 md[p][r])) + add,   r = state_row[j]
//   E[p][j]  = multiply ? E[p][j] * f[p][j] : f[p][j]
//
// The reference materialises a (rows, b*L, d) difference tensor on the way; here the only traffic is
// the embedding columns (read once, in place, from a tensor whose rows are `ld` floats apart) and E.
//
// The distance is evaluated in the difference form, not as [x, x^2] against a table: the expanded
// form is a GEMM, but it cancels whenever |x - mean| << |mean| (trained class means lie many sigmas
// apart and an embedding sits next to one of them), and it is exactly that row whose factor matters.
// The difference form needs 3 VALU operations per (position, row, column) — rows * 3/4 per input
// byte, which for the 13 rows of the 15-state model stays below the machine's VALU : HBM ratio.
//
// Shape of the kernel.  A workgroup of MV_THREADS lanes owns MV_THREADS consecutive positions, one
// per lane, and walks the d columns in slices of MV_KS:
//   load   the slice of all positions, 16 bytes per lane (4 lanes per 64-byte row segment), into
//          registers one slice ahead, then into LDS — the row-per-lane read below would otherwise
//          touch a cache line per lane and instruction;
//   sum    lane p reads its MV_KS floats back (row stride MV_KS + 4: conflict-free 16-byte reads) and
//          runs over the rows; mean / inv_std of a row are wave-uniform, so they arrive through the
//          scalar cache and feed the VALU as scalar operands: no table staging, no LDS reads
//          in the inner loop.  Four partial sums per row and slice, then md[r][p] in LDS (+=).
//   flush  lane p turns md[.][p] into f in place; then the tile of E — MV_THREADS * q contiguous
//          floats — is walked flat in 16-byte pieces, each element finding its (position, state) by
//          a multiply-high and its factor in LDS.  With multiply, E is read and written once.
// LDS: MV_THREADS * (MV_KS + 4) + rows * (MV_THREADS + 1) floats + q ints: 34 KB for 13 rows, 54 KB at
// the limit of 32.  No workspace, no atomics, no dependence on the grid: results are deterministic.
// The load / sum walk is mv_md, shared with the backward (hmm_emitter_mvn_grad.inc) and with the kernels for up to 256
// states (hmm_emitter_mvn_wide.inc, hmm_emitter_mvn_grad_wide.inc), which run it per block of 32 rows.
// Compiler figures (gfx950, hipcc -O3): 70 VGPRs, no scratch.

#define MV_MAXQ 64
#define MV_MAXR 32
#define MV_MAXD 4096
#define MV_THREADS 256
#define MV_KS 16                      // columns per slice
#define MV_XS (MV_KS + 4)             // LDS row stride of the staged slice, floats
#define MV_FS (MV_THREADS + 1)        // LDS row stride of md / f, floats

struct MvSlice { f4 v[MV_KS / 4]; };

// the slice [k0, k0 + MV_KS) of positions [P0, P0 + MV_THREADS): piece i of lane tid is columns
// 4 c4 .. 4 c4 + 3 of position (tid + i * MV_THREADS) / (MV_KS / 4).  Columns from d on and positions
// from npos on are never read and arrive as 0.
__device__ __forceinline__ MvSlice mv_load(const float *__restrict__ emb, long long ld, long long npos, int d,
                                           long long P0, int k0, int tid) {
    MvSlice sl;
#pragma unroll
    for (int i = 0; i < MV_KS / 4; ++i) {
        const int ch = tid + i * MV_THREADS;
        const int p = ch / (MV_KS / 4), c = k0 + 4 * (ch % (MV_KS / 4));
        const long long pos = P0 + p;
        f4 v = {0.f, 0.f, 0.f, 0.f};
        if (pos < npos) {
            const float *src = emb + pos * ld + c;
            if (c + 4 <= d) {
                v = *reinterpret_cast<const f4u *>(src);
            } else {
                if (c < d) v.x = src[0];
                if (c + 1 < d) v.y = src[1];
                if (c + 2 < d) v.z = src[2];
            }
        }
        sl.v[i] = v;
    }
    return sl;
}

// Slice sl covers columns [k0, k0 + MV_KS).  The last slice of a d that is no multiple of MV_KS is moved
// back to end at d, so that every slice of a d >= MV_KS is whole (one 64-byte scalar load per table and
// row); its first sl * MV_KS - k0 columns were summed by the slice before and are masked out.
__device__ __forceinline__ int mv_k0(int sl, int d) {
    const int k0 = sl * MV_KS;
    return k0 + MV_KS <= d || d < MV_KS ? k0 : d - MV_KS;
}

// md[r] (+)= sum over the slice's columns, for every row.  mean / inv_std point at the slice's first
// column of row 0 and are wave-uniform: a row's 2 x MV_KS values arrive by two 64-byte scalar loads and feed
// the VALU as scalar operands; two rows per iteration share one wait.  Four partial sums per row.
template <bool MASKED>
__device__ __forceinline__ void mv_sum(const float (&xr)[MV_KS], const float *__restrict__ mean,
                                       const float *__restrict__ inv_std, int d, int rows, int skip, float *fcol,
                                       bool first) {
#pragma unroll 2
    for (int r = 0; r < rows; ++r) {
        const float *m = mean + (size_t)r * d, *s = inv_std + (size_t)r * d;
        float a[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < MV_KS; ++c) {
            const float t = (xr[c] - m[c]) * (MASKED && c < skip ? 0.f : s[c]);
            a[c & 3] = fmaf(t, t, a[c & 3]);
        }
        const float part = (a[0] + a[1]) + (a[2] + a[3]);
        fcol[r * MV_FS] = first ? part : fcol[r * MV_FS] + part;
    }
}

// d < MV_KS: one partial slice; the tables are read below column d only, the lane's row from LDS
__device__ __forceinline__ void mv_sum_narrow(const float *xrow, const float *__restrict__ mean,
                                              const float *__restrict__ inv_std, int d, int rows, float *fcol) {
#pragma unroll 1
    for (int r = 0; r < rows; ++r) {
        float a = 0.f;
#pragma unroll 1
        for (int c = 0; c < d; ++c) {
            const float t = (xrow[c] - mean[r * d + c]) * inv_std[r * d + c];
            a = fmaf(t, t, a);
        }
        fcol[r * MV_FS] = a;
    }
}

// srow[q] (clamped), rstart[rows + 1], rlist[q]: states of row r are rlist[rstart[r] .. rstart[r + 1]), ascending
__device__ __forceinline__ void mv_row_lists(const int *__restrict__ state_row, int q, int rows, int *srow, int *rstart,
                                              int *rlist, int tid) {
    for (int j = tid; j < q; j += MV_THREADS) {
        const int r = state_row[j];
        srow[j] = r < 0 ? 0 : (r < rows ? r : rows - 1);
    }
    __syncthreads();
    for (int r = tid; r <= rows; r += MV_THREADS) {
        int n = 0;
        for (int j = 0; j < q; ++j) n += srow[j] < r;
        rstart[r] = n;
        if (r < rows)
            for (int j = 0; j < q; ++j)
                if (srow[j] == r) rlist[n++] = j;
    }
    __syncthreads();
}

// The walk over the d columns of tile P0 for rows [r0, r0 + nr), shared by the forward and backward kernels of both
// widths (the 64-state ones pass r0 = 0, nr = rows): md into fs[0 .. nr)[tid].  pre holds the tile's first slice on
// entry and the first slice of tile Pnext (if Pnext >= 0) on exit.
__device__ __forceinline__ void mv_md(const float *__restrict__ emb, long long ld, long long npos, int d,
                                       const float *__restrict__ mean, const float *__restrict__ inv_std, int r0, int nr,
                                       long long P0, long long Pnext, MvSlice &pre, float *xs, float *fs, int tid) {
    const int nslices = (d + MV_KS - 1) / MV_KS;
    const float *mb = mean + (size_t)r0 * d, *sb = inv_std + (size_t)r0 * d;
    for (int sl = 0; sl < nslices; ++sl) {
        const int k0 = mv_k0(sl, d), skip = sl * MV_KS - k0;
        __syncthreads();                                  // the previous slice's readers / the previous item's flush are done
#pragma unroll
        for (int i = 0; i < MV_KS / 4; ++i) {
            const int ch = tid + i * MV_THREADS;
            *reinterpret_cast<f4 *>(xs + (ch / (MV_KS / 4)) * MV_XS + 4 * (ch % (MV_KS / 4))) = pre.v[i];
        }
        __syncthreads();
        // one slice ahead: the next slice of this tile, or the first of tile Pnext.  One call site on purpose: with one
        // per case the compiler keeps both sets of row addresses alive, which costs k_embedding_emissions a wave per SIMD
        const bool last = sl + 1 == nslices;
        if (!last || Pnext >= 0) pre = mv_load(emb, ld, npos, d, last ? Pnext : P0, last ? 0 : mv_k0(sl + 1, d), tid);

        float xr[MV_KS];
#pragma unroll
        for (int i = 0; i < MV_KS / 4; ++i) {
            const f4 v = *reinterpret_cast<const f4 *>(xs + tid * MV_XS + 4 * i);
            xr[4 * i] = v.x; xr[4 * i + 1] = v.y; xr[4 * i + 2] = v.z; xr[4 * i + 3] = v.w;
        }
        if (d < MV_KS) mv_sum_narrow(xs + tid * MV_XS, mb, sb, d, nr, fs + tid);
        else if (skip == 0) mv_sum<false>(xr, mb + k0, sb + k0, d, nr, 0, fs + tid, sl == 0);
        else mv_sum<true>(xr, mb + k0, sb + k0, d, nr, skip, fs + tid, false);
    }
}

__global__ __launch_bounds__(MV_THREADS) void k_embedding_emissions(const float *__restrict__ emb, long long ld,
                                                                    long long npos, int d,
                                                                    const float *__restrict__ mean,
                                                                    const float *__restrict__ inv_std,
                                                                    const float *__restrict__ log_norm, int rows,
                                                                    const int *__restrict__ state_row, int q,
                                                                    float inv_temperature, float add, int multiply,
                                                                    float *__restrict__ E) {
    extern __shared__ __attribute__((aligned(16))) float mv_lds[];
    float *xs = mv_lds;                                   // [MV_THREADS][MV_XS]
    float *fs = xs + MV_THREADS * MV_XS;                  // [rows][MV_FS]: md, then f
    int *srow = reinterpret_cast<int *>(fs + rows * MV_FS);     // [q]
    const int tid = threadIdx.x;
    if (tid < q) {
        const int r = state_row[tid];
        srow[tid] = r < 0 ? 0 : (r < rows ? r : rows - 1);
    }
    // e / q == umulhi(e, ceil(2^32 / q)) for e < 2^14 and 2 <= q <= 64: the excess e * (q - 1) / (q * 2^32) stays below 1/q
    const unsigned qmagic = (unsigned)((0x100000000ull + (unsigned)q - 1u) / (unsigned)q);
    const long long ntiles = (npos + MV_THREADS - 1) / MV_THREADS;

    long long tile = blockIdx.x;
    if (tile >= ntiles) return;
    MvSlice pre = mv_load(emb, ld, npos, d, tile * MV_THREADS, 0, tid);
    for (; tile < ntiles; tile += gridDim.x) {
        const long long P0 = tile * MV_THREADS;
        mv_md(emb, ld, npos, d, mean, inv_std, 0, rows, P0, tile + gridDim.x < ntiles ? (tile + gridDim.x) * MV_THREADS : -1, pre,
              xs, fs, tid);
        // md -> f, in place (lane p owns column p of fs)
#pragma unroll 1
        for (int r = 0; r < rows; ++r)
            fs[r * MV_FS + tid] = expf(inv_temperature * (log_norm[r] - 0.5f * fs[r * MV_FS + tid])) + add;
        __syncthreads();
        // the tile of E, flat
        const long long left = npos - P0;
        const int nfl = (int)(left < MV_THREADS ? left : MV_THREADS) * q;     // floats that exist, <= 2^14
        float *dst = E + P0 * q;
        for (int e0 = 4 * tid; e0 < nfl; e0 += 4 * MV_THREADS) {
            float f[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const unsigned e = (unsigned)(e0 + u) < (unsigned)nfl ? (unsigned)(e0 + u) : (unsigned)(nfl - 1);
                const unsigned p = q == 1 ? e : __umulhi(e, qmagic);
                f[u] = fs[srow[e - p * (unsigned)q] * MV_FS + p];
            }
            if (e0 + 4 <= nfl) {
                f4 v = {f[0], f[1], f[2], f[3]};
                if (multiply) { const f4 old = *reinterpret_cast<const f4u *>(dst + e0); v *= old; }
                *reinterpret_cast<f4u *>(dst + e0) = v;
            } else {
                for (int u = 0; e0 + u < nfl; ++u) dst[e0 + u] = multiply ? dst[e0 + u] * f[u] : f[u];
            }
        }
    }
}

extern "C" int hmm_embedding_emissions_max_dim(void) { return MV_MAXD; }

extern "C" int hmm_embedding_emissions(const float *emb, long long ld, int b, int L, int d, const float *mean,
                                       const float *inv_std, const float *log_norm, int rows, const int *state_row,
                                       int q, float inv_temperature, float add, int multiply, float *E, void *stream) {
    if (b < 1 || L < 1 || d < 1 || rows < 1 || q < 1 || ld < d) return HMM_ERR_BAD_SHAPE;
    if (q > MV_MAXQ || rows > MV_MAXR || d > MV_MAXD) return HMM_ERR_Q_UNSUPPORTED;
    if (!emb || !mean || !inv_std || !log_norm || !state_row || !E) return HMM_ERR_NULL_POINTER;
    if (multiply != 0 && multiply != 1) return HMM_ERR_BAD_ARGUMENT;
    const long long npos = (long long)b * L;
    const long long ntiles = (npos + MV_THREADS - 1) / MV_THREADS;
    const size_t lds = ((size_t)MV_THREADS * MV_XS + (size_t)rows * MV_FS) * sizeof(float) + (size_t)q * sizeof(int);
    const dim3 grid((unsigned)(ntiles < 256 * 16 ? ntiles : 256 * 16));
    hipLaunchKernelGGL(k_embedding_emissions, grid, dim3(MV_THREADS), lds, (hipStream_t)stream, emb, ld, npos, d, mean,
                       inv_std, log_norm, rows, state_row, q, inv_temperature, add, multiply, E);
    return check_launch();
}
