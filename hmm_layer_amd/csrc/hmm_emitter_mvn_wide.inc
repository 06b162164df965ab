// hmm_emitter_mvn_wide.inc — the embedding-emission factor (hmm_emitter_mvn.inc) for up to 256 states and 256
// kernel rows: the gene models of three to eighteen copies.  Included by hmm_engine.hip after hmm_emitter_mvn.inc,
// whose helpers (mv_load, mv_md, mv_row_lists) it calls unchanged.  Same arguments, layouts and formulas:
//
//   md[p][r] = sum_c ((x[p][c] - mean[r][c]) * inv_std[r][c])^2
//   f[p][j]  = exp(inv_temperature * (log_norm[r] - 0.5 md[p][r])) + add,   r = state_row[j]
//   E[p][j]  = multiply ? E[p][j] * f[p][j] : f[p][j]
//
// evaluated in the difference form (DESIGN §10b: the expanded form cancels on the row that matters).
//
// The 64-state kernel keeps md of all rows of a 256-position tile in LDS, fs[rows][257]: 263 KB at 256 rows.  Here
// the rows are cut into blocks of MVW_RB = 32.  A work item is (tile of 256 positions, row block); the items are
// dealt to the workgroups round-robin.  An item is the 64-state kernel's tile walk restricted to its rows:
//   load / sum   as hmm_emitter_mvn.inc (slices of 16 columns, staged through LDS, lane = position, the tables as
//          scalar operands; mv_sum with the tables offset to the block's first row).  The embedding slice of a
//          tile is read once per row block, from L2 after the first.
//   flush  lane p turns md[.][p] of the block into f in place.  The states whose row lies in the block are
//          rlist[rstart[r0] .. rstart[r0 + nr]) (states sorted by row, ascending within a row; built once per
//          workgroup).  They are walked in chunks of 32: lane = (position p = e / 32, list entry e % 32), so that
//          a position's 32 states are neighbours in the wave (one 128-byte segment of E for an identity map).
//          Every element of E is touched by exactly one item, once.
// Per (position, row) the summation order over d is that of the 64-state kernel (slices in order, four partial sums
// per slice), so wherever both accept a shape the outputs are bit-identical.
// LDS: 256 * 20 + 32 * 257 floats + 2 q + rows + 1 ints: 53.4 KB + at most 3 KB.  No workspace, no atomics, no
// dependence on the grid.
//
// Compiler figures (gfx950, hipcc -O3): see DESIGN §10e.

#define MVW_MAXQ 256
#define MVW_MAXR 256
#define MVW_RB 32                     // rows per block
#define MVW_SC 32                     // states per chunk of the flush
#define MVW_MAXGRID 1024

__global__ __launch_bounds__(MV_THREADS) void k_embedding_emissions_wide(const float *__restrict__ emb, long long ld,
                                                                         long long npos, int d,
                                                                         const float *__restrict__ mean,
                                                                         const float *__restrict__ inv_std,
                                                                         const float *__restrict__ log_norm, int rows,
                                                                         const int *__restrict__ state_row, int q,
                                                                         float inv_temperature, float add, int multiply,
                                                                         float *__restrict__ E) {
    extern __shared__ __attribute__((aligned(16))) float mv_lds[];
    float *xs = mv_lds;                                   // [MV_THREADS][MV_XS]
    float *fs = xs + MV_THREADS * MV_XS;                  // [MVW_RB][MV_FS]: md, then f, of the item's rows
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
        // md -> f, in place (lane p owns column p of fs)
#pragma unroll 1
        for (int r = 0; r < nr; ++r)
            fs[r * MV_FS + tid] = expf(inv_temperature * (log_norm[r0 + r] - 0.5f * fs[r * MV_FS + tid])) + add;
        __syncthreads();
        // the block's states, 32 at a time; 8 positions per pass of the workgroup
        const int kend = rstart[r0 + nr];
        const int kk = tid & (MVW_SC - 1);
        for (int kc = rstart[r0]; kc < kend; kc += MVW_SC) {
            if (kc + kk >= kend) continue;
            const int j = rlist[kc + kk];
            const float *frow = fs + (srow[j] - r0) * MV_FS;
            for (int p = tid / MVW_SC; p < MV_THREADS; p += MV_THREADS / MVW_SC) {
                const long long pos = P0 + p;
                if (pos >= npos) break;
                float *dst = E + pos * q + j;
                const float f = frow[p];
                *dst = multiply ? f * *dst : f;
            }
        }
    }
}

extern "C" int hmm_embedding_emissions_wide_max_states(void) { return MVW_MAXQ; }

static size_t mvw_lds_bytes(int stage_floats, int rows, int q) {
    return ((size_t)stage_floats + (size_t)MVW_RB * MV_FS) * sizeof(float) + (size_t)(2 * q + rows + 1) * sizeof(int);
}

static unsigned mvw_grid(long long npos, int rows) {
    const long long nitems = ((npos + MV_THREADS - 1) / MV_THREADS) * ((rows + MVW_RB - 1) / MVW_RB);
    return (unsigned)(nitems < MVW_MAXGRID ? nitems : MVW_MAXGRID);
}

extern "C" int hmm_embedding_emissions_wide(const float *emb, long long ld, int b, int L, int d, const float *mean,
                                            const float *inv_std, const float *log_norm, int rows,
                                            const int *state_row, int q, float inv_temperature, float add, int multiply,
                                            float *E, void *stream) {
    if (b < 1 || L < 1 || d < 1 || rows < 1 || q < 1 || ld < d) return HMM_ERR_BAD_SHAPE;
    if (q > MVW_MAXQ || rows > MVW_MAXR || d > MV_MAXD) return HMM_ERR_Q_UNSUPPORTED;
    if (!emb || !mean || !inv_std || !log_norm || !state_row || !E) return HMM_ERR_NULL_POINTER;
    if (multiply != 0 && multiply != 1) return HMM_ERR_BAD_ARGUMENT;
    const long long npos = (long long)b * L;
    hipLaunchKernelGGL(k_embedding_emissions_wide, dim3(mvw_grid(npos, rows)), dim3(MV_THREADS),
                       mvw_lds_bytes(MV_THREADS * MV_XS, rows, q), (hipStream_t)stream, emb, ld, npos, d, mean, inv_std,
                       log_norm, rows, state_row, q, inv_temperature, add, multiply, E);
    return check_launch();
}
