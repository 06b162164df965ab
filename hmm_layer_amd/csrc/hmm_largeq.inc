// hmm_largeq.inc — forward / backward / posterior for q > 16 states (profile-HMM sizes,
// BASELINE config 5: q = 2*512+3 = 1027), included by hmm_engine.hip.
//
// A scan over q x q operators costs q^3 per position, so large models run serial in time exactly
// as the reference does (hmm_layer/BaseRNN.py:217-227 over hmm_layer/MsaHmmCell.py:73-106) — but
// each step is ONE f32-MFMA GEMM over the whole batch, R = X A (forward) or R = X A^T (backward)
// [the reference's per-step torch.matmul, hmm_layer/gene_pred_hmm_transitioner.py:122-125], with the
// cell's exact clamp / emission / normalise / log semantics (hmm_layer/MsaHmmCell.py:87-103) fused into
// the GEMM's epilogue in both directions: one launch per position and direction.  Row sums are
// per-tile partials added in a fixed order (deterministic).  The posterior runs the two recursions
// at the same time on two streams, from both ends towards the middle and on through each other's
// half (lq_posterior): until they meet each parks its vector in the output tensor itself, afterwards
// each multiplies its vector into what the other parked; one elementwise pass normalises at the end.
// No L-sized workspace.

#define LQ_BM 64
#define LQ_BK 32
#define LQ_LD (LQ_BK + 4)      // LDS row stride in floats (16-byte multiple)
#define LQ_THREADS 512

// R[M][N=q] = X[M][K=q] (row stride ldx) * Bt^T, Bt is q x q row-major with K contiguous: Bt = A^T for
// the forward direction (x A, transposed once per call by k_lq_transpose) and A itself for the
// backward direction (x A^T).
// Tile: 64 rows x BN = 16 NTW columns, BN chosen on the host so that every CU gets at most one tile
// where possible (q = 1027, b = 1024: 64 x 80 -> 208 tiles; 64 x 64 would be 272 tiles, i.e. a
// two-deep critical path on 16 CUs).  512 threads = 8 waves: wave w owns the 16-row strip w & 3 over
// the full tile width and the 16-wide half w >> 2 of every 32-wide K slab (two waves per SIMD hide
// each other's LDS latency); the two K-halves are added through LDS in a fixed order at the end.
// Both operands sit in LDS with K contiguous and are read with the k-permutation of the scan kernels:
// lane (g, r) supplies k = 4g + kk at MFMA step kk, so ONE ds_read_b128 feeds four MFMAs.  Slabs are
// double-buffered: one barrier per slab, the next slab's global loads in flight under the MFMAs.
// Tile map: workgroups are dealt round-robin to the 8 XCDs, so XCD x = (mg, ng) owns a compact
// mper x nper block of tiles (4 x 2 blocks cover the matrix) and its L2 holds just those panels.
// Epilogue: the cell step fused into the GEMM — no second launch per position.  The operand X is the
// UNNORMALISED previous vector (forward: U_{t-1} = max(E,eps) * max(R,eps); backward: V_{t+1} = max(E,eps) * Rb);
// its row sums come as per-tile partials (Pprev[row][tile], summed here in a fixed order), so that
// r = max(acc / S, eps) is the normalised, clamped vector the cell defines.  The tile writes the next operand
// (forward U_t = E'_t r, backward V_t = E'_t r) with its own partial row sums, and
//   lg   (or null)  log alpha_t = log U_t + ll_{t-1}  |  log beta_t = log r + lscale_t   (ll / lscale are
//                   double-buffered: tile column 0 writes llcur = llprev + log S, every tile derives the same)
//   park (or null)  COMBINE ? park * val : val,  val = U_t (forward) | r = Rb_t (backward): what the posterior
//                   keeps in its output tensor (see lq_posterior)
// Nothing downstream ever wants the normalised alpha_hat: log alpha needs no S_t (ll_t = ll_{t-1} + log S_t
// cancels it) and the posteriors are scale-free in it.
__device__ __forceinline__ float lq_block_sum(float v, float *red);
#define LQ_NTP 64                // row stride of the partial sums: at most 4096 / 64 tile columns
struct LqStep {
    const float *E;              // E[:, t, :], row stride lde
    long long lde;
    const float *Pprev;          // [row][LQ_NTP]
    float *Pcur;
    const double *llprev;        // [row]
    double *llcur;
    float *nxt;                  // next operand, row stride ldn
    long long ldn;
    float *lg;                   // log output or null, row stride ldl
    long long ldl;
    float *park;                 // output tensor row block or null, row stride ldp
    long long ldp;
    float eps;
    int NT;                      // tile columns of the previous step's partials
    int sign;                    // park with the sign bit set where the clamp of r was active (acc / S <= eps):
                                 // the live bit hmm_loglik_grad_large's adjoint recursion reads
};

template <int NTW, bool BWD, bool COMBINE>
__global__ __launch_bounds__(LQ_THREADS) void k_lq_gemm(const float *__restrict__ X, long long ldx,
                                                        const float *__restrict__ Bt, int q, int M,
                                                        int mper, int nper, LqStep fw) {
    constexpr int BN = 16 * NTW;
    constexpr int NB4 = BN * (LQ_BK / 4);                 // 16-byte pieces of one B slab
    constexpr bool TWO = NB4 > LQ_THREADS;
    __shared__ __attribute__((aligned(16))) float Xs[2][LQ_BM][LQ_LD];
    __shared__ __attribute__((aligned(16))) float Bs[2][BN][LQ_LD];
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const int tm = (xcd >> 1) * mper + slot / nper, tn = (xcd & 1) * nper + slot % nper;
    if (slot >= mper * nper || tm * LQ_BM >= M || tn * BN >= q) return;     // uniform for the block, before any barrier
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int strip = w & 3, kh = w >> 2;
    const int m0 = tm * LQ_BM, n0 = tn * BN;
    const int g = lane >> 4, n16 = lane & 15;
    __shared__ float sinv[LQ_BM], slln[LQ_BM];
    if (tid < LQ_BM) {
        // 1 / S and ll (lscale) of this tile's rows (the main loop's first barrier publishes them)
        const int row = min(m0 + tid, M - 1);
        float S = 0.f;
        for (int u = 0; u < fw.NT; ++u) S += fw.Pprev[(size_t)row * LQ_NTP + u];
        const double lln = fw.llprev[row] + (double)logf(S);
        sinv[tid] = 1.0f / S;
        slln[tid] = (float)lln;
        if (tn == 0 && m0 + tid < M) fw.llcur[row] = lln;
    }
    f4 acc[NTW];
#pragma unroll
    for (int j = 0; j < NTW; ++j) acc[j] = (f4){0.f, 0.f, 0.f, 0.f};
    // the epilogue's emission values are requested now and used after the last slab: their latency sits
    // under the whole product instead of at its end (the K-half 0 waves write the tile)
    f4 ev[NTW], pv[COMBINE ? NTW : 1];
    if (kh == 0) {
#pragma unroll
        for (int j = 0; j < NTW; ++j) {
            const int col = min(n0 + j * 16 + n16, q - 1);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = min(m0 + strip * 16 + 4 * g + r, M - 1);
                ev[j][r] = fw.E[(long long)row * fw.lde + col];
                if (COMBINE) pv[j][r] = fw.park[(long long)row * fw.ldp + col];
            }
        }
    }

    // staging: thread -> one 16-byte piece of the X slab (64 rows x 8 pieces) and one or two of the B
    // slab.  Rows past M / q are clamped to valid memory: their products land in accumulator rows /
    // columns that are never stored.  Full slabs are loaded with no guards at all — a branch around a
    // load makes the compiler wait for it on the spot, which serialised loads and MFMAs.
    const int xr = tid >> 3, pk = (tid & 7) * 4;
    const float *xrow = X + (long long)min(m0 + xr, M - 1) * ldx;
    const int br0 = tid >> 3, br1 = (tid + LQ_THREADS) >> 3;             // B rows of this thread's pieces
    const bool has0 = tid < NB4, has1 = TWO && tid + LQ_THREADS < NB4;
    const float *brow0 = Bt + (long long)min(n0 + (has0 ? br0 : 0), q - 1) * q;
    const float *brow1 = Bt + (long long)min(n0 + (has1 ? br1 : 0), q - 1) * q;
    auto load4_tail = [&](const float *ptr, int first) -> f4 {      // last, partial slab only
        f4 v = {0.f, 0.f, 0.f, 0.f};
        if (first < q) v.x = ptr[first];
        if (first + 1 < q) v.y = ptr[first + 1];
        if (first + 2 < q) v.z = ptr[first + 2];
        if (first + 3 < q) v.w = ptr[first + 3];
        return v;
    };
    auto load4 = [&](const float *ptr) -> f4 {
        const P4 t = *reinterpret_cast<const P4 *>(ptr);
        return (f4){t.a, t.b, t.c, t.d};
    };
    struct Regs { f4 x, b0, b1; };
    auto fetch = [&](int k0) {
        Regs r;
        r.x = r.b0 = r.b1 = (f4){0.f, 0.f, 0.f, 0.f};
        if (k0 + LQ_BK <= q) {                               // wave-uniform
            r.x = load4(xrow + k0 + pk);
            r.b0 = load4(brow0 + k0 + pk);
            if (TWO) r.b1 = load4(brow1 + k0 + pk);
        } else if (k0 < q) {
            r.x = load4_tail(xrow, k0 + pk);
            r.b0 = load4_tail(brow0, k0 + pk);
            if (TWO) r.b1 = load4_tail(brow1, k0 + pk);
        }
        return r;
    };
    auto store = [&](int buf, const Regs &r) {
        *reinterpret_cast<f4 *>(&Xs[buf][xr][pk]) = r.x;
        if (has0) *reinterpret_cast<f4 *>(&Bs[buf][br0][pk]) = r.b0;
        if (has1) *reinterpret_cast<f4 *>(&Bs[buf][br1][pk]) = r.b1;
    };
    auto compute = [&](int buf) {
        const f4 a = *reinterpret_cast<const f4 *>(&Xs[buf][strip * 16 + n16][kh * 16 + 4 * g]);
        f4 b[NTW];
#pragma unroll
        for (int j = 0; j < NTW; ++j) b[j] = *reinterpret_cast<const f4 *>(&Bs[buf][j * 16 + n16][kh * 16 + 4 * g]);
        // kk outermost: consecutive MFMAs go to different accumulators (a dependent chain on one
        // accumulator issues every ~40 cycles instead of 32)
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
#pragma unroll
            for (int j = 0; j < NTW; ++j)
                acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[kk], b[j][kk], acc[j], 0, 0, 0);
    };
    // Measured on MI355X (q = 1027, b = 1024, tools/experiments/largeq_variants.py): this loop 32 us;
    // the same MFMAs with no LDS / loads / barrier 24 us (the floor of this tiling: 208 of 256 CUs,
    // ~2.0 GHz sustained matrix clock).  Keeping operand fragments one slab ahead in registers, or
    // three slabs of global loads in flight, changed nothing, so the loop stays simple.
    const int nslab = (q + LQ_BK - 1) / LQ_BK;
    Regs rg = fetch(0);
    store(0, rg);
    __syncthreads();
    for (int sl = 0; sl < nslab; ++sl) {
        const int buf = sl & 1;
        if (sl + 1 < nslab) rg = fetch((sl + 1) * LQ_BK);
        compute(buf);
        if (sl + 1 < nslab) store(buf ^ 1, rg);
        __syncthreads();
    }
    // add the two K-halves (fixed order: low half + high half) and store
    float *red = &Bs[0][0][0];                               // 64 x BN floats fit in the B buffers
    if (kh == 1) {
#pragma unroll
        for (int j = 0; j < NTW; ++j) *reinterpret_cast<f4 *>(red + ((strip * NTW + j) * 64 + lane) * 4) = acc[j];
    }
    __syncthreads();
    if (kh == 0) {
        float rsum[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < NTW; ++j) {
            const f4 o = *reinterpret_cast<const f4 *>(red + ((strip * NTW + j) * 64 + lane) * 4);
            const int col = n0 + j * 16 + n16;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int rl = strip * 16 + 4 * g + r, row = m0 + rl;
                if (row < M && col < q) {
                    const float rraw = (acc[j][r] + o[r]) * sinv[rl];
                    const float rr = fmaxf(rraw, fw.eps);
                    const float sf = fmaxf(ev[j][r], fw.eps) * rr;
                    const float val = BWD ? rr : sf;
                    fw.nxt[(long long)row * fw.ldn + col] = sf;
                    if (fw.lg) fw.lg[(long long)row * fw.ldl + col] = logf(val) + slln[rl];
                    if (fw.park) {
                        const float pk = COMBINE ? val * pv[j][r] : val;
                        fw.park[(long long)row * fw.ldp + col] = (fw.sign && !(rraw > fw.eps)) ? -pk : pk;
                    }
                    rsum[r] += sf;
                }
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float s16 = row_sum_f(rsum[r]);               // over the 16 lanes that share (strip, g): fixed order
            const int row = m0 + strip * 16 + 4 * g + r;
            if (n16 == 0 && row < M) fw.Pcur[(size_t)row * LQ_NTP + tn] = s16;
        }
    }
}

// first position of a recursion.  Forward (pi given): U_0 = max(E_0,eps) * max(pi,eps); backward (pi null):
// Rb = ones, V = max(E,eps).  The row sum is the single partial, ll = 0.
__global__ __launch_bounds__(256) void k_lq_init(const float *__restrict__ pi, const float *__restrict__ E,
                                                 long long lde, float *__restrict__ nxt, long long ldn,
                                                 float *__restrict__ lg, long long ldl, float *__restrict__ park,
                                                 long long ldp, int combine, float *__restrict__ P,
                                                 double *__restrict__ ll, int q, int b, float eps) {
    __shared__ float red[4];
    const int row = blockIdx.x, m = row / b;
    const float *Er = E + (long long)row * lde;
    float part = 0.f;
    for (int j = threadIdx.x; j < q; j += 256) {
        const float r = pi ? fmaxf(pi[(size_t)m * q + j], eps) : 1.f;
        const float sf = fmaxf(Er[j], eps) * r;
        const float val = pi ? sf : r;
        nxt[(long long)row * ldn + j] = sf;
        if (lg) lg[(long long)row * ldl + j] = logf(val);
        if (park) park[(long long)row * ldp + j] = combine ? val * park[(long long)row * ldp + j] : val;
        part += sf;
    }
    const float S = lq_block_sum(part, red);
    for (int u = threadIdx.x; u < LQ_NTP; u += 256) P[(size_t)row * LQ_NTP + u] = u == 0 ? S : 0.f;
    if (threadIdx.x == 0) ll[row] = 0.0;
}

// after the last position of the forward recursion: loglik = ll_{L-2} + log S_{L-1}
__global__ __launch_bounds__(256) void k_lq_fwd_finish(const float *__restrict__ P, const double *__restrict__ llprev,
                                                       double *__restrict__ ll, int NB, int NT) {
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= NB) return;
    float S = 0.f;
    for (int u = 0; u < NT; ++u) S += P[(size_t)row * LQ_NTP + u];
    ll[row] = llprev[row] + (double)logf(S);
}

// At[m] = A[m]^T (q x q), 32 x 32 tiles through LDS
__global__ __launch_bounds__(256) void k_lq_transpose(const float *__restrict__ A, float *__restrict__ At, int q) {
    __shared__ float tile[32][33];
    const size_t mo = (size_t)blockIdx.z * q * q;
    const int x0 = blockIdx.x * 32, y0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int r = ty; r < 32; r += 8)
        if (y0 + r < q && x0 + tx < q) tile[r][tx] = A[mo + (size_t)(y0 + r) * q + x0 + tx];
    __syncthreads();
    for (int r = ty; r < 32; r += 8)
        if (x0 + r < q && y0 + tx < q) At[mo + (size_t)(x0 + r) * q + y0 + tx] = tile[tx][r];
}

// deterministic block sum (256 threads), result broadcast to all
__device__ __forceinline__ float lq_block_sum(float v, float *red) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[w] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// posterior: out[row][t][:] holds g = U_t * Rb_t (any scale); one block per (row, t):
//   mode 0: g / sum g    1: log g - log sum g    2: log g - log sum g + loglik
#define LQ_NORM_PER 20           // states per thread held in registers: q <= 256 * 20 covers HMM_LARGEQ_MAX
__global__ __launch_bounds__(256) void k_lq_normalise(float *__restrict__ out, long long L, int q, int mode,
                                                      const double *__restrict__ loglik) {
    __shared__ float red[4];
    const long long rt = blockIdx.x;                         // row * L + t
    float *o = out + rt * q;
    float v[LQ_NORM_PER];
    float part = 0.f;
#pragma unroll
    for (int u = 0; u < LQ_NORM_PER; ++u) {
        const int j = threadIdx.x + u * 256;
        v[u] = j < q ? o[j] : 0.f;
        part += v[u];
    }
    const float Sg = lq_block_sum(part, red);
    const float ig = 1.0f / Sg;
    const float sh = mode == 0 ? 0.f : logf(Sg);
    // mode 2: the three terms are added in double and rounded once.  Added in float, the result carried three half
    // ulps of |loglik| (1.4e-3 at |loglik| = 8400, L = 3000) instead of one.
    const double shd = mode == 2 ? (double)sh - loglik[rt / L] : 0.0;
#pragma unroll
    for (int u = 0; u < LQ_NORM_PER; ++u) {
        const int j = threadIdx.x + u * 256;
        if (j < q) o[j] = mode == 0 ? v[u] * ig : mode == 1 ? logf(v[u]) - sh : (float)((double)logf(v[u]) - shd);
    }
}

#define LQ_SP_BYTES 8208            // sizeof(MqSp), hmm_midq.inc (asserted there)
struct LqPlan {
    int k, b, L, q, NB;
    size_t o_X0, o_X1, o_V0, o_V1, o_ll, o_At, o_P, o_ll2, o_Pb, o_ls2, o_sp, total;
};

static int make_lqplan(int k, int b, int L, int q, LqPlan *p) {
    if (k < 1 || b < 1 || L < 1 || q < 1) return HMM_ERR_BAD_SHAPE;
    if (q > HMM_LARGEQ_MAX) return HMM_ERR_Q_UNSUPPORTED;
    if (q > 256 * LQ_NORM_PER) return HMM_ERR_Q_UNSUPPORTED;
    p->k = k; p->b = b; p->L = L; p->q = q; p->NB = k * b;
    size_t off = 0;
    const size_t mat = (size_t)p->NB * q * sizeof(float);
    p->o_X0 = off; off = align_up(off + mat);              // forward operands U_t, ping-pong
    p->o_X1 = off; off = align_up(off + mat);
    p->o_V0 = off; off = align_up(off + mat);              // backward operands V_t, ping-pong
    p->o_V1 = off; off = align_up(off + mat);
    p->o_ll = off; off = align_up(off + (size_t)p->NB * sizeof(double));
    p->o_At = off; off = align_up(off + (size_t)k * q * q * sizeof(float));
    p->o_P = off;  off = align_up(off + 2 * (size_t)p->NB * LQ_NTP * sizeof(float));       // forward partial row sums, two steps
    p->o_ll2 = off; off = align_up(off + 2 * (size_t)p->NB * sizeof(double));             // running loglik, two steps
    p->o_Pb = off; off = align_up(off + 2 * (size_t)p->NB * LQ_NTP * sizeof(float));       // the same for the backward recursion
    p->o_ls2 = off; off = align_up(off + 2 * (size_t)p->NB * sizeof(double));
    p->o_sp = off;  off = align_up(off + (q <= 64 ? (size_t)k * LQ_SP_BYTES : 0));        // 17..64 states: the sparse-step tables (MqSp)
    p->total = off;
    return HMM_OK;
}

// one GEMM per model: X rows [m*b, (m+1)*b) times Bt[m]^T.  Tile width: the one with the cheapest
// critical path, (tiles per CU, rounded up) x width, on 256 CUs.
// tile width (in 16-column units) of the GEMM instantiation serving (b, q): 4, 5 or 6
static int lq_tile_width(int b, int q) {
    const int MT = (b + LQ_BM - 1) / LQ_BM;
    int best = 4;
    long long best_cost = -1;
    // (a 128-column tile can only ever tie with the 64-column one under this rule: tiles(4) <= 2 tiles(8))
    for (int ntw = 4; ntw <= 6; ++ntw) {
        const long long tiles = (long long)MT * ((q + 16 * ntw - 1) / (16 * ntw));
        const long long cost = ((tiles + 255) / 256) * ntw;
        if (best_cost < 0 || cost < best_cost) { best = ntw; best_cost = cost; }
    }
    return best;
}
static int lq_tile_cols(const LqPlan &p) {
    const int w = 16 * lq_tile_width(p.b, p.q);
    return (p.q + w - 1) / w;
}

// one fused step (LqStep; per-model row offsets are applied here)
static void lq_gemm(const float *X, long long ldx, const float *Bt, const LqPlan &p, hipStream_t st, const LqStep &fw,
                    bool bwd, bool combine) {
    const int MT = (p.b + LQ_BM - 1) / LQ_BM;
    const int best = lq_tile_width(p.b, p.q);
    const int NT = (p.q + 16 * best - 1) / (16 * best);
    const int mper = (MT + 3) / 4, nper = (NT + 1) / 2;
    const dim3 grid(8 * mper * nper);
    for (int m = 0; m < p.k; ++m) {
        const float *Xm = X + (long long)m * p.b * ldx, *Bm = Bt + (size_t)m * p.q * p.q;
        LqStep f = fw;
        const long long r0 = (long long)m * p.b;
        f.E += r0 * f.lde; f.Pprev += r0 * LQ_NTP; f.Pcur += r0 * LQ_NTP; f.llprev += r0; f.llcur += r0;
        f.nxt += r0 * f.ldn;
        if (f.lg) f.lg += r0 * f.ldl;
        if (f.park) f.park += r0 * f.ldp;
#define LQ_LAUNCH2(NTW_, B_, C_) \
        hipLaunchKernelGGL((k_lq_gemm<NTW_, B_, C_>), grid, dim3(LQ_THREADS), 0, st, Xm, ldx, Bm, p.q, p.b, mper, nper, f)
#define LQ_LAUNCH(NTW_) \
        do { \
            if (!bwd && !combine) LQ_LAUNCH2(NTW_, false, false); \
            else if (!bwd) LQ_LAUNCH2(NTW_, false, true); \
            else if (!combine) LQ_LAUNCH2(NTW_, true, false); \
            else LQ_LAUNCH2(NTW_, true, true); \
        } while (0)
        switch (best) {
            case 4: LQ_LAUNCH(4); break;
            case 5: LQ_LAUNCH(5); break;
            default: LQ_LAUNCH(6); break;
        }
#undef LQ_LAUNCH
#undef LQ_LAUNCH2
    }
}

// One recursion as a sequence of launches on one stream.  A step at position t either parks its vector
// (forward: U_t, backward: Rb_t) or multiplies it into what the other recursion parked there.
struct LqChain {
    bool bwd;
    const float *Bt;             // forward: A^T (k_lq_transpose); backward: A
    float *buf[2];               // next-operand ping-pong (row stride q)
    float *P;                    // partial row sums, two steps
    double *ll2;                 // running log scale, two steps
    const float *Xprev;          // operand of the next step
    long long ldprev;
    int NTprev, steps;
};
static LqChain lq_chain(bool bwd, const float *Bt, const LqPlan &p, char *ws) {
    LqChain c;
    c.bwd = bwd; c.Bt = Bt;
    c.buf[0] = (float *)(ws + (bwd ? p.o_V0 : p.o_X0)); c.buf[1] = (float *)(ws + (bwd ? p.o_V1 : p.o_X1));
    c.P = (float *)(ws + (bwd ? p.o_Pb : p.o_P));
    c.ll2 = (double *)(ws + (bwd ? p.o_ls2 : p.o_ll2));
    c.Xprev = nullptr; c.ldprev = 0; c.NTprev = 1; c.steps = 0;
    return c;
}
// nxt_in_place: the next operand is written to the output tensor itself (forward recursion parking U_t),
// otherwise to the chain's ping-pong buffers
static void lq_step(LqChain &c, int t, const float *pi, const float *E, const LqPlan &p, float eps, float *lg,
                    float *park, bool combine, float *nxt_in_place, hipStream_t st) {
    const long long ldt = (long long)p.L * p.q;
    const int i = c.steps & 1;
    float *Pcur = c.P + (size_t)i * p.NB * LQ_NTP, *Pprev = c.P + (size_t)(i ^ 1) * p.NB * LQ_NTP;
    double *llcur = c.ll2 + (size_t)i * p.NB, *llprev = c.ll2 + (size_t)(i ^ 1) * p.NB;
    float *nxt = nxt_in_place ? nxt_in_place + (long long)t * p.q : c.buf[i];
    const long long ldn = nxt_in_place ? ldt : p.q;
    float *lgt = lg ? lg + (long long)t * p.q : nullptr, *pk = park ? park + (long long)t * p.q : nullptr;
    if (c.steps == 0) {
        hipLaunchKernelGGL(k_lq_init, dim3(p.NB), dim3(256), 0, st, c.bwd ? (const float *)nullptr : pi,
                           E + (long long)t * p.q, ldt, nxt, ldn, lgt, ldt, pk, ldt, combine ? 1 : 0, Pcur, llcur, p.q, p.b,
                           eps);
    } else {
        LqStep f = {E + (long long)t * p.q, ldt, Pprev, Pcur, llprev, llcur, nxt, ldn, lgt, ldt, pk, ldt, eps, c.NTprev};
        lq_gemm(c.Xprev, c.ldprev, c.Bt, p, st, f, c.bwd, combine);
        c.NTprev = lq_tile_cols(p);
    }
    c.Xprev = nxt; c.ldprev = ldn;
    ++c.steps;
}
static void lq_finish_loglik(const LqChain &c, const LqPlan &p, char *ws, hipStream_t st) {
    const int last = (c.steps - 1) & 1;
    hipLaunchKernelGGL(k_lq_fwd_finish, dim3((p.NB + 255) / 256), dim3(256), 0, st,
                       (const float *)(c.P + (size_t)last * p.NB * LQ_NTP), (const double *)(c.ll2 + (size_t)last * p.NB),
                       (double *)(ws + p.o_ll), p.NB, c.NTprev);
}
static float *lq_transposed(const float *A, const LqPlan &p, char *ws, hipStream_t st) {
    float *At = (float *)(ws + p.o_At);
    hipLaunchKernelGGL(k_lq_transpose, dim3((p.q + 31) / 32, (p.q + 31) / 32, p.k), dim3(256), 0, st, A, At, p.q);
    return At;
}

// forward over all positions: log alpha (or null) and loglik -> ws + o_ll
static void lq_forward(const float *A, const float *pi, const float *E, const LqPlan &p, float eps, char *ws,
                       float *log_alpha, hipStream_t st) {
    LqChain f = lq_chain(false, lq_transposed(A, p, ws, st), p, ws);
    for (int t = 0; t < p.L; ++t) lq_step(f, t, pi, E, p, eps, log_alpha, nullptr, false, nullptr, st);
    lq_finish_loglik(f, p, ws, st);
}

// backward over all positions: log beta
static void lq_backward(const float *A, const float *E, const LqPlan &p, float eps, char *ws, float *log_beta,
                        hipStream_t st) {
    LqChain b = lq_chain(true, A, p, ws);
    for (int t = p.L - 1; t >= 0; --t) lq_step(b, t, nullptr, E, p, eps, log_beta, nullptr, false, nullptr, st);
}

// Posterior.  The two recursions are independent until they need each other's vector, and one GEMM per
// position leaves the machine half idle (208 of 256 CUs, one workgroup each, launch to launch), so they run
// AT THE SAME TIME on two streams (measured: two independent chains take 1.6x the time of one, not 2x):
//   until they meet (h = ceil(L/2))   forward t = 0 .. h-1 parks U_t in out[:, t, :] (and reads it back from
//                                     there as its next operand); backward t = L-1 .. h parks Rb_t
//   afterwards                        forward t = h .. L-1 stores U_t * (parked Rb_t); backward t = h-1 .. 0
//                                     stores (parked U_t) * Rb_t
// and one elementwise pass normalises every (row, t) (k_lq_normalise; needs the forward recursion's loglik in
// mode 2).  `side` = a second stream or null (then everything runs in order on st: same results).
static void lq_posterior(const float *A, const float *pi, const float *E, const LqPlan &p, float eps, char *ws,
                         float *out, int mode, hipStream_t st, hipStream_t side) {
    LqChain f = lq_chain(false, lq_transposed(A, p, ws, st), p, ws), b = lq_chain(true, A, p, ws);
    const int h = (p.L + 1) / 2;
    hipStream_t sb = side ? side : st;
    hipEvent_t ev[4];
    if (side) {
        for (int i = 0; i < 4; ++i) (void)hipEventCreateWithFlags(&ev[i], hipEventDisableTiming);
        (void)hipEventRecord(ev[0], st);                     // fork (after the transpose and whatever preceded the call)
        (void)hipStreamWaitEvent(side, ev[0], 0);
    }
    // (the last parked U_t also goes to the ping-pong buffer: the backward recursion overwrites out[:, h-1, :]
    // while the forward one still reads it as its operand)
    for (int t = 0; t < h; ++t) lq_step(f, t, pi, E, p, eps, nullptr, t == h - 1 ? out : nullptr, false, t == h - 1 ? nullptr : out, st);
    for (int t = p.L - 1; t >= h; --t) lq_step(b, t, nullptr, E, p, eps, nullptr, out, false, nullptr, sb);
    if (side) {
        (void)hipEventRecord(ev[1], st);
        (void)hipEventRecord(ev[2], side);
        (void)hipStreamWaitEvent(st, ev[2], 0);
        (void)hipStreamWaitEvent(side, ev[1], 0);
    }
    for (int t = h; t < p.L; ++t) lq_step(f, t, pi, E, p, eps, nullptr, out, true, nullptr, st);
    for (int t = h - 1; t >= 0; --t) lq_step(b, t, nullptr, E, p, eps, nullptr, out, true, nullptr, sb);
    lq_finish_loglik(f, p, ws, st);
    if (side) {
        (void)hipEventRecord(ev[3], side);
        (void)hipStreamWaitEvent(st, ev[3], 0);
        for (int i = 0; i < 4; ++i) (void)hipEventDestroy(ev[i]);
    }
    hipLaunchKernelGGL(k_lq_normalise, dim3((unsigned)((long long)p.NB * p.L)), dim3(256), 0, st, out, (long long)p.L, p.q,
                       mode, (const double *)(ws + p.o_ll));
}
