// hmm_emitter_nuc.inc — trainable nucleotide factor of the gene-prediction models
// (trainable_nucleotides_at_exons=True), forward and backward, included by hmm_engine.hip.  Replaces the acgt
// einsum, the (b, L, q) concatenation with the 1/4 columns and the product of GenePredHMMEmitter.forward
// (hmm_layer/gene_pred_hmm_emitter.py:224-229, 265-272):
//
//   acgt[p][a] = nuc[p][a] + nuc[p][4] / 4                            a = 0..3
//   f[p][j]    = r >= 0 ? sum_a acgt[p][a] * P[r][a] : free_value,    r = state_nuc[j] (>= rows: rows - 1)
//   E[p][j]    = multiply ? E[p][j] * f[p][j] : f[p][j]
//
// and, with dE = dL/dE_out,
//
//   dE_in[p][j] = dE[p][j] * f[p][j]
//   dP[r][a]    = sum_p acgt[p][a] * sum_{j: state_nuc[j] = r} dE[p][j] * E_in[p][j]
//
// There is no division: an all-zero nucleotide row (padding) gives f = 0 and finite gradients.  The five
// nucleotide floats of a position are read in place from a tensor whose rows are `ld` floats apart; nothing
// else of that tensor is touched.  Per value: the acgt add (nuc[4] / 4 is exact), one multiply and three fmas
// in the order a = 0, 1, 2, 3, and the product with E — six rounded operations at the most.
//
// k_nucleotide_emissions.  A workgroup of NE_THREADS lanes owns tiles of NE_THREADS consecutive positions:
//   stage  lane p turns its position's five floats into acgt[p] (one 16-byte LDS slot);
//   walk   the tile of E — NE_THREADS * q contiguous floats — is walked flat in 16-byte pieces, each element
//          finding its (position, state) by a multiply-high, acgt[p] and its state's row of P in LDS.  The
//          per-state tables (row of P, free flag) are kept at slot (j & 3) * 64 + j / 4: the lanes of a wave
//          hold states 4 apart for the same piece element, which lands them on consecutive 16-byte slots.
//          With multiply, E is read and written once.
// LDS: 4 KB acgt + 4 KB rows of P + 1 KB flags.  No workspace, no atomics, nothing depends on the grid.
//
// k_nucleotide_emissions_grad.  One pass over dE (and E_in), each byte read once.  Lane = (position group g,
// state j) with G = NE_THREADS / q groups (17 for the 15-state model, 1 above 128 states); the lanes walk a
// tile in steps of G positions, G * q contiguous floats per step and stream (dE, E_in, dE_in), eight steps in
// flight; the next tile's nucleotides are loaded one tile ahead.  A lane keeps its state's row of P and its
// four dP accumulators in registers; acgt[p] is staged as in the forward and read as a broadcast.  E_in is read
// on the states with a row only.  dE_in leaves at once.  Reduction order of dP, fixed by (b L, q,
// rows, state_nuc) alone: workgroup x of X = min(tiles, 1024) takes tiles x, x + X, ...; lane (g, j) adds its
// positions in ascending order (fp32, one fma each); at the end element (r, a) of the workgroup's partial is
// the sum over the states j of row r in ascending order, and for each state over g in ascending order (fp32);
// k_nucleotide_emissions_grad_sum adds the partials in workgroup order in fp64 and rounds once.  Every kernel
// computes the same values whatever is stored, so calls for either output alone are bit-identical.
// LDS: 4 KB acgt + 4 KB accumulators + 1 KB row map.  Workspace: X partials of rows * 4 floats (at most 4 MiB).
//
// Compiler figures (gfx950, hipcc -O3): k_nucleotide_emissions 43 VGPRs (8 waves per SIMD),
// k_nucleotide_emissions_grad 77 (6 waves; its 1024 workgroups fill 4), k_nucleotide_emissions_grad_sum 24;
// no scratch in any of them, 9216 bytes of LDS in the first two.

#define NE_MAXQ 256
#define NE_MAXR 256
#define NE_THREADS 256                // lanes per workgroup = positions per tile
#define NE_MAXBLOCKS 1024             // workgroup partials the sum kernel adds
#define NE_STEPS 8                    // steps of the backward walk whose loads are in flight together

// acgt of position pos; positions from npos on arrive as 0
__device__ __forceinline__ f4 ne_acgt(const float *__restrict__ nuc, long long ld, long long npos, long long pos) {
    f4 v = {0.f, 0.f, 0.f, 0.f};
    if (pos < npos) {
        const float *src = nuc + pos * ld;
        const float n4 = 0.25f * src[4];
        v.x = src[0] + n4; v.y = src[1] + n4; v.z = src[2] + n4; v.w = src[3] + n4;
    }
    return v;
}

__device__ __forceinline__ float ne_dot(const f4 a, const f4 p) {
    return fmaf(a.w, p.w, fmaf(a.z, p.z, fmaf(a.y, p.y, a.x * p.x)));
}

__device__ __forceinline__ int ne_row(int r, int rows) { return r < 0 ? -1 : (r < rows ? r : rows - 1); }

__global__ __launch_bounds__(NE_THREADS) void k_nucleotide_emissions(const float *__restrict__ nuc, long long ld,
                                                                     long long npos, const float *__restrict__ P,
                                                                     int rows, const int *__restrict__ state_nuc, int q,
                                                                     float free_value, int multiply,
                                                                     float *__restrict__ E) {
    __shared__ f4 as[NE_THREADS];                         // acgt of the tile
    __shared__ f4 ps[NE_MAXQ];                            // state j's row of P at slot (j & 3) * 64 + j / 4
    __shared__ int sfree[NE_MAXQ];                        // same slots: 1 for a free state
    const int tid = threadIdx.x;
    if (tid < q) {
        const int r = ne_row(state_nuc[tid], rows);
        const int slot = ((tid & 3) << 6) | (tid >> 2);
        f4 v = {0.f, 0.f, 0.f, 0.f};
        if (r >= 0) v = *reinterpret_cast<const f4u *>(P + 4 * r);
        ps[slot] = v;
        sfree[slot] = r < 0;
    }
    // e / q == umulhi(e, ceil(2^32 / q)) for e < 2^16 and 2 <= q <= 256: the excess e * (q - 1) / (q * 2^32) stays below 1/q
    const unsigned qmagic = (unsigned)((0x100000000ull + (unsigned)q - 1u) / (unsigned)q);
    const long long ntiles = (npos + NE_THREADS - 1) / NE_THREADS;

    for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long long P0 = tile * NE_THREADS;
        __syncthreads();                                  // the previous tile's walk is done (first tile: nothing)
        as[tid] = ne_acgt(nuc, ld, npos, P0 + tid);
        __syncthreads();                                  // acgt complete (first tile: the tables too)
        const long long left = npos - P0;
        const int nfl = (int)(left < NE_THREADS ? left : NE_THREADS) * q;     // floats that exist, <= 2^16
        float *dst = E + P0 * q;
        for (int e0 = 4 * tid; e0 < nfl; e0 += 4 * NE_THREADS) {
            float f[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const unsigned e = (unsigned)(e0 + u) < (unsigned)nfl ? (unsigned)(e0 + u) : (unsigned)(nfl - 1);
                const unsigned p = q == 1 ? e : __umulhi(e, qmagic);
                const unsigned j = e - p * (unsigned)q;
                const unsigned slot = ((j & 3u) << 6) | (j >> 2);
                const float dot = ne_dot(as[p], ps[slot]);
                f[u] = sfree[slot] ? free_value : dot;
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

__global__ __launch_bounds__(NE_THREADS) void k_nucleotide_emissions_grad(
    const float *__restrict__ nuc, long long ld, long long npos, const float *__restrict__ P, int rows,
    const int *__restrict__ state_nuc, int q, float free_value, const float *__restrict__ E_in,
    const float *__restrict__ dE, float *__restrict__ dE_in, float *__restrict__ part) {
    __shared__ f4 as[NE_THREADS];                         // acgt of the tile
    __shared__ f4 accs[NE_THREADS];                       // the lanes' accumulators, for the partial
    __shared__ int srow[NE_MAXQ];
    const int tid = threadIdx.x;
    const int G = NE_THREADS / q;                         // position groups, >= 1
    const int g = tid / q, j = tid - g * q;
    const bool active = g < G;
    const int r = active ? ne_row(state_nuc[j], rows) : -1;
    f4 pj = {0.f, 0.f, 0.f, 0.f};
    if (r >= 0) pj = *reinterpret_cast<const f4u *>(P + 4 * r);
    f4 acc = {0.f, 0.f, 0.f, 0.f};
    const long long ntiles = (npos + NE_THREADS - 1) / NE_THREADS;

    f4 pre = ne_acgt(nuc, ld, npos, (long long)blockIdx.x * NE_THREADS + tid);
    for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long long P0 = tile * NE_THREADS;
        __syncthreads();                                  // the previous tile's readers are done
        as[tid] = pre;
        __syncthreads();
        pre = ne_acgt(nuc, ld, npos, P0 + (long long)gridDim.x * NE_THREADS + tid);    // the next tile's, one tile ahead
        const long long left = npos - P0;
        const int cnt = (int)(left < NE_THREADS ? left : NE_THREADS);
        if (!active) continue;                            // no barrier below
        const long long base = P0 * q + j;
        for (int p0 = g; p0 < cnt; p0 += NE_STEPS * G) {
            float gv[NE_STEPS], ev[NE_STEPS];
#pragma unroll
            for (int u = 0; u < NE_STEPS; ++u) {          // eight steps' loads in flight
                const int p = p0 + u * G;
                const long long off = base + (long long)p * q;
                gv[u] = p < cnt ? dE[off] : 0.f;
                ev[u] = (p < cnt && E_in && r >= 0) ? E_in[off] : 1.f;
            }
#pragma unroll
            for (int u = 0; u < NE_STEPS; ++u) {
                const int p = p0 + u * G;
                if (p < cnt) {
                    const f4 a = as[p];
                    const float f = r >= 0 ? ne_dot(a, pj) : free_value;
                    if (dE_in) dE_in[base + (long long)p * q] = gv[u] * f;
                    const float h = r >= 0 ? gv[u] * ev[u] : 0.f;
                    acc.x = fmaf(a.x, h, acc.x); acc.y = fmaf(a.y, h, acc.y);
                    acc.z = fmaf(a.z, h, acc.z); acc.w = fmaf(a.w, h, acc.w);
                }
            }
        }
    }
    if (!part) return;
    // the workgroup's partial: element (row, a) = its states in ascending order, per state the groups in order
    accs[tid] = acc;
    if (tid < q) srow[tid] = r;                           // g == 0: tid == j
    __syncthreads();
    const float *af = reinterpret_cast<const float *>(accs);
    float *dst = part + (size_t)blockIdx.x * rows * 4;
    for (int idx = tid; idx < rows * 4; idx += NE_THREADS) {
        const int rr = idx >> 2, a = idx & 3;
        float sum = 0.f;
        for (int s = 0; s < q; ++s)
            if (srow[s] == rr)
                for (int k = 0; k < G; ++k) sum += af[4 * (k * q + s) + a];
        dst[idx] = sum;
    }
}

// the partials in workgroup order, fp64, rounded once
__global__ __launch_bounds__(64) void k_nucleotide_emissions_grad_sum(const float *__restrict__ part, int nblk, int nel,
                                                                      float *__restrict__ dP) {
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (e >= nel) return;
    double sum = 0.0;
#pragma unroll 16
    for (int k = 0; k < nblk; ++k) sum += (double)part[(size_t)k * nel + e];       // 16 loads in flight, added in order
    dP[e] = (float)sum;
}

static int neg_blocks(long long npos) {
    const long long ntiles = (npos + NE_THREADS - 1) / NE_THREADS;
    return (int)(ntiles < NE_MAXBLOCKS ? ntiles : NE_MAXBLOCKS);
}

extern "C" int hmm_nucleotide_emissions_max_states(void) { return NE_MAXQ; }

extern "C" int hmm_nucleotide_emissions(const float *nuc, long long ld, int b, int L, const float *P, int rows,
                                        const int *state_nuc, int q, float free_value, int multiply, float *E,
                                        void *stream) {
    if (b < 1 || L < 1 || q < 1 || rows < 1 || ld < 5) return HMM_ERR_BAD_SHAPE;
    if (q > NE_MAXQ || rows > NE_MAXR) return HMM_ERR_Q_UNSUPPORTED;
    if (!nuc || !P || !state_nuc || !E) return HMM_ERR_NULL_POINTER;
    if (multiply != 0 && multiply != 1) return HMM_ERR_BAD_ARGUMENT;
    const long long npos = (long long)b * L;
    const long long ntiles = (npos + NE_THREADS - 1) / NE_THREADS;
    const dim3 grid((unsigned)(ntiles < 256 * 16 ? ntiles : 256 * 16));
    hipLaunchKernelGGL(k_nucleotide_emissions, grid, dim3(NE_THREADS), 0, (hipStream_t)stream, nuc, ld, npos, P, rows,
                       state_nuc, q, free_value, multiply, E);
    return check_launch();
}

// min(tiles, 1024) workgroup partials of rows * 4 floats: at most 4 MiB, whatever b*L
extern "C" size_t hmm_nucleotide_emissions_grad_workspace_bytes(int b, int L, int rows, int q) {
    if (b < 1 || L < 1 || q < 1 || rows < 1 || q > NE_MAXQ || rows > NE_MAXR) return 0;
    const size_t bytes = (size_t)neg_blocks((long long)b * L) * rows * 4 * sizeof(float);
    return (bytes + 255) & ~(size_t)255;
}

extern "C" int hmm_nucleotide_emissions_grad(const float *nuc, long long ld, int b, int L, const float *P, int rows,
                                             const int *state_nuc, int q, float free_value, const float *E_in,
                                             const float *dE, float *dE_in, float *dP, void *workspace,
                                             size_t workspace_bytes, void *stream) {
    if (b < 1 || L < 1 || q < 1 || rows < 1 || ld < 5) return HMM_ERR_BAD_SHAPE;
    if (q > NE_MAXQ || rows > NE_MAXR) return HMM_ERR_Q_UNSUPPORTED;
    if (!nuc || !P || !state_nuc || !dE || !workspace || (!dE_in && !dP)) return HMM_ERR_NULL_POINTER;
    if (workspace_bytes < hmm_nucleotide_emissions_grad_workspace_bytes(b, L, rows, q) || ((uintptr_t)workspace & 255))
        return HMM_ERR_WORKSPACE;
    const long long npos = (long long)b * L;
    const int nblk = neg_blocks(npos);
    float *part = dP ? (float *)workspace : nullptr;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_nucleotide_emissions_grad, dim3((unsigned)nblk), dim3(NE_THREADS), 0, st, nuc, ld, npos, P, rows,
                       state_nuc, q, free_value, E_in, dE, dE_in, part);
    if (dP)
        hipLaunchKernelGGL(k_nucleotide_emissions_grad_sum, dim3((unsigned)((rows * 4 + 63) / 64)), dim3(64), 0, st, part,
                           nblk, rows * 4, dP);
    return check_launch();
}
