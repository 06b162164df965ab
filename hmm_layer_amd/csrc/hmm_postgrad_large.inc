// hmm_postgrad_large.inc — gradient of a loss on the state posteriors for 1 <= q <= 4096 states
// (hmm_posterior_grad_large), included after hmm_postgrad.inc and hmm_grad_large.inc.
//
// The derivatives, modes and clamp handling of hmm_postgrad.inc (DESIGN §12): with the values
//   forward   u_t = E'_t max(R^f_t, eps),  R^f_t = t ? alpha_hat_{t-1} A : pi,  alpha_hat_t = u_t / S_t
//   backward  Rb_{L-1} = 1,  Rb_t = max(A bh_{t+1}, eps),  bh_t = E'_t Rb_t / Sb_t
//   output    g_t = alpha_hat_t Rb_t,  gamma_t = g_t / Sg_t,  out_t = gamma_t | log gamma_t
// the adjoint of the backward recursion runs forward in time (w_t = live(Rb_t) Rbar_t, dA += w_t (x) bh_{t+1},
// bhbar = A^T w_t, through the normalisation of bh_{t+1} to dE_{t+1} and Rbar_{t+1}) and the adjoint of the forward
// recursion runs backward in time (through the normalisation of u_t to dE_t and Rfbar_t, dA += alpha_hat_{t-1} (x)
// Rfbar_t, abar_{t-1} = A Rfbar_t, dpi at t = 0).  pg_local's trick stays: gbar * alpha and gbar * Rb are formed
// directly, so log mode never divides by an underflowed posterior.
//
// The value sweeps store the UNNORMALISED forward vector U_t = u_t (sign bit: the forward clamp was active) and Rb_t
// (sign bit: the backward clamp was active), k*b*L*q floats each; the adjoints normalise U_t themselves.  dE of the
// backward recursion's adjoint is parked in the caller's dE, that of the forward recursion's in the workspace, and
// k_pg_merge adds them where E was not clamped.  Sums run in a fixed order: fp32 within a sequence or a tile, fp64
// across sequences (k_pg_grad_sum, k_pg_sum_rows) and positions (the fp64 accumulator of k_gl_dA).
//
// Kernels:
//   k_gl_walk_fwd, k_pgl_walk_rb<QB>, k_pgl_walk_beta<QB>, k_pgl_walk_alpha<QB>   per-sequence walk
//                 (HMM_OPT_GLARGE = 1, default for q <= GL_Q_WALK): one workgroup per sequence, ceil(q/64) waves,
//                 lane = state, A or A^T in LDS, the vector of the step in LDS, cross-wave sums meeting in LDS in a
//                 fixed order.  The value sweeps need one barrier per step; each adjoint step needs two (the
//                 normalisation adjoint's dot product depends on the step's own mat-vec).  Lane i holds row i of the
//                 sequence's dA partial in registers.
//   k_lq_gemm + k_pgl_beta_step / k_pgl_alpha_step + k_gl_dA   per-position GEMMs (HMM_OPT_GLARGE = 2, default
//                 above GL_Q_WALK, valid for every q): the value recursions are hmm_largeq.inc's forward and backward
//                 steps parking signed values (LqStep.sign); each adjoint step is one k_lq_gemm in the other
//                 orientation run as a plain product (unit emissions, unit row sums, eps = -inf: the epilogue passes
//                 the product through unchanged), one block per sequence for the normalisation adjoints, dE and the
//                 masking, and one k_gl_dA outer product (K = sequences) into the fp64 k q^2 accumulator.

struct PglLayout {
    LqPlan lq;                    // the GEMM route's value recursions and operands (hmm_largeq.inc), at offset 0
    size_t o_ah, o_rb, o_dea, o_s, o_ll, o_dpi, o_rf, o_ap, o_ab, o_ones, o_acc, o_gpart, o_gpart2, total;
};

static void pgl_layout(int k, int b, int L, int q, PglLayout *g) {
    make_lqplan(k, b, L, q, &g->lq);
    const size_t nr = (size_t)k * b, seq = nr * L * q * sizeof(float), vec = nr * q * sizeof(float);
    const size_t gp = q <= GL_WALK_MAX ? nr * q * q * sizeof(float) : 0;
    size_t off = g->lq.total;
    g->o_ah = off;     off = align_up(off + seq);                                 // signed U_t
    g->o_rb = off;     off = align_up(off + seq);                                 // signed Rb_t
    g->o_dea = off;    off = align_up(off + seq);                                 // dE through the forward recursion
    g->o_s = off;      off = align_up(off + nr * L * sizeof(float));              // walk: S_t
    g->o_ll = off;     off = align_up(off + nr * sizeof(double));
    g->o_dpi = off;    off = align_up(off + vec);                                 // dpi per sequence
    g->o_rf = off;     off = align_up(off + vec);                                 // GEMMs: Rfbar_t
    g->o_ap = off;     off = align_up(off + vec);                                 //        alpha_hat_{t-1}
    g->o_ab = off;     off = align_up(off + vec);                                 //        abar_{t-1} = A Rfbar_t
    g->o_ones = off;   off = align_up(off + (size_t)q * sizeof(float));
    g->o_acc = off;    off = align_up(off + (size_t)k * q * q * sizeof(double));  // dA in fp64
    g->o_gpart = off;  off = align_up(off + gp);                                  // walk: dA partials per sequence
    g->o_gpart2 = off; off = align_up(off + gp);
    g->total = off;
}

// d loss / d g (g = alpha_hat Rb) times alpha_hat (ga: into Rbar) and times Rb (gr: into abar), from the row sums
// Sg = sum g, SGg = sum G g, SG = sum G (pg_local with the sums given)
__device__ __forceinline__ void pgl_local(float G, float al, float rb, bool act, int mode, float Sg, float SGg,
                                          float SG, float *ga, float *gr) {
    const float ig = 1.0f / Sg;
    if (mode == 0) {
        const float gb = act ? (G - SGg * ig) * ig : 0.f;
        *ga = gb * al;
        *gr = gb * rb;
    } else {
        const float c = SG * ig;
        *ga = act ? (rb > 0.f ? G / rb : 0.f) - c * al : 0.f;
        *gr = act ? (al > 0.f ? G / al : 0.f) - c * rb : 0.f;
    }
}
// sum over the lanes of gr * al, from the same sums (SGp = sum of G where al > 0): zero in exact arithmetic
__device__ __forceinline__ float pgl_gr_dot_al(int mode, float Sg, float SGg, float SG, float SGp) {
    const float ig = 1.0f / Sg;
    return mode == 0 ? ig * (SGg - (SGg * ig) * Sg) : SGp - SG * ig * Sg;
}

// per-wave partials of N sums -> LDS; every lane reads the totals back (wave 0 + wave 1, fixed order)
template <int N, int NW>
__device__ __forceinline__ void pgl_publish(const float (&v)[N], float (*red)[2]) {
    const int w = threadIdx.x >> 6;
#pragma unroll
    for (int x = 0; x < N; ++x) {
        const float s = gl_wave_sum(v[x]);
        if ((threadIdx.x & 63) == 0) red[x][w] = s;
    }
}
template <int N, int NW>
__device__ __forceinline__ void pgl_collect(float (*red)[2], float (&v)[N]) {
#pragma unroll
    for (int x = 0; x < N; ++x) v[x] = NW == 1 ? red[x][0] : red[x][0] + red[x][1];
}

// ------------------------------------------------------------------ per-sequence walk
// backward value sweep: grid k*b, block QB; dynamic LDS At[j][i] = A[i][j] (row stride QB).  RB_t = Rb_t signed.
template <int QB>
__global__ __launch_bounds__(QB) void k_pgl_walk_rb(const float *__restrict__ A, const float *__restrict__ E, int b,
                                                    int L, int q, float eps, float *__restrict__ RB) {
    extern __shared__ float At[];
    __shared__ __attribute__((aligned(16))) float xs[2][QB];
    __shared__ float ws[2][2];
    constexpr int NW = QB / 64;
    const long long row = blockIdx.x;
    const int m = (int)(row / b), i = threadIdx.x, w = i >> 6;
    const int q4 = (q + 3) & ~3;
    const bool act = i < q;
    const float *Am = A + (size_t)m * q * q;
    for (int jj = 0; jj < q4; ++jj) At[jj * QB + i] = (act && jj < q) ? Am[(size_t)i * q + jj] : 0.f;
    const float *Er = E + (size_t)row * L * q;
    float *o = RB + (size_t)row * L * q;
    float en = act ? Er[(size_t)(L - 1) * q + i] : 0.f;
    __syncthreads();                                          // At staged
    for (int t = L - 1; t >= 0; --t) {
        const float eraw = en;
        if (t > 0 && act) en = Er[(size_t)(t - 1) * q + i];
        float rb = 1.f;
        bool live = true;
        if (t < L - 1) {
            const int cur = (t + 1) & 1;
            const float S = NW == 1 ? ws[cur][0] : ws[cur][0] + ws[cur][1];
            float a[4] = {0.f, 0.f, 0.f, 0.f};
            for (int jj = 0; jj < q4; jj += 4) {
                const f4 v = *reinterpret_cast<const f4 *>(&xs[cur][jj]);
                a[0] = fmaf(At[jj * QB + i], v.x, a[0]);
                a[1] = fmaf(At[(jj + 1) * QB + i], v.y, a[1]);
                a[2] = fmaf(At[(jj + 2) * QB + i], v.z, a[2]);
                a[3] = fmaf(At[(jj + 3) * QB + i], v.w, a[3]);
            }
            const float raw = ((a[0] + a[1]) + (a[2] + a[3])) / S;
            live = raw > eps;
            rb = fmaxf(raw, eps);
        }
        if (act) o[(size_t)t * q + i] = live ? rb : -rb;
        const float sb = act ? fmaxf(eraw, eps) * rb : 0.f;
        xs[t & 1][i] = sb;
        const float s = gl_wave_sum(sb);
        if ((i & 63) == 0) ws[t & 1][w] = s;
        __syncthreads();
    }
}

// adjoint of the backward recursion, ascending in time: grid k*b, block QB; dynamic LDS As[i][x] = A[i][x]
// (row stride QB).  Writes dEb (d loss / d E' through bh, every position) and the sequence's dA partial
// sum_t w_t (x) bh_{t+1}, row x in lane x.
template <int QB>
__global__ __launch_bounds__(QB) void k_pgl_walk_beta(const float *__restrict__ A, const float *__restrict__ E,
                                                      const float *__restrict__ AH, const float *__restrict__ Sst,
                                                      const float *__restrict__ RB, const float *__restrict__ G, int b,
                                                      int L, int q, float eps, int mode, float *__restrict__ dEb,
                                                      float *__restrict__ gpart) {
    extern __shared__ float As[];
    __shared__ __attribute__((aligned(16))) float wv[QB];
    __shared__ __attribute__((aligned(16))) float sv[QB];
    __shared__ float r0[3][2], r1[4][2], r2[1][2];
    constexpr int NW = QB / 64;
    const long long row = blockIdx.x;
    const int m = (int)(row / b), x = threadIdx.x;
    const int q4 = (q + 3) & ~3;
    const bool act = x < q;
    const float *Am = A + (size_t)m * q * q;
    for (int i = 0; i < q4; ++i) As[i * QB + x] = (act && i < q) ? Am[(size_t)i * q + x] : 0.f;
    const size_t base = (size_t)row * L * q;
    const float *Sr = Sst + (size_t)row * L;
    auto ld = [&](const float *p, int t) { return act ? p[base + (size_t)t * q + x] : 0.f; };
    float grow[QB];
#pragma unroll
    for (int j = 0; j < QB; ++j) grow[j] = 0.f;
    // position 0: Rbar_0 from its own output term only; bh_0 feeds nothing
    float rbs = ld(RB, 0), Rbar;
    {
        const float al = __builtin_fabsf(ld(AH, 0)) / Sr[0], rb = __builtin_fabsf(rbs), Gt = ld(G, 0);
        const float g = act ? al * rb : 0.f;
        const float v[3] = {g, act ? Gt * g : 0.f, Gt};
        pgl_publish<3, NW>(v, r0);
        __syncthreads();                                      // As staged, sums of position 0
        float s[3];
        pgl_collect<3, NW>(r0, s);
        float gr;
        pgl_local(Gt, al, rb, act, mode, s[0], s[1], s[2], &Rbar, &gr);
        if (act) dEb[base + x] = 0.f;
    }
    float ne = 0.f, nr = 0.f, na = 0.f, ng = 0.f, ns = 0.f;  // position t + 1, loaded a step ahead
    if (L > 1) { ne = ld(E, 1); nr = ld(RB, 1); na = ld(AH, 1); ng = ld(G, 1); ns = Sr[1]; }
    for (int t = 0; t + 1 < L; ++t) {
        const float e1 = fmaxf(ne, eps), rb1s = nr, al1 = __builtin_fabsf(na) / ns, G1 = ng;
        if (t + 2 < L) { ne = ld(E, t + 2); nr = ld(RB, t + 2); na = ld(AH, t + 2); ng = ld(G, t + 2); ns = Sr[t + 2]; }
        const float rb1 = __builtin_fabsf(rb1s);
        const float wx = (act && __builtin_bit_cast(int, rbs) >= 0) ? Rbar : 0.f;   // the clamp of Rb_t passes nothing
        const float sb = act ? e1 * rb1 : 0.f, g1 = act ? al1 * rb1 : 0.f;
        wv[x] = wx;
        sv[x] = sb;
        const float v[4] = {sb, g1, act ? G1 * g1 : 0.f, G1};
        pgl_publish<4, NW>(v, r1);
        __syncthreads();
        float s[4];
        pgl_collect<4, NW>(r1, s);
        const float iSb = 1.0f / s[0], coef = wx * iSb;
        float a[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j0 = 0; j0 < QB; j0 += 4) {
            if (j0 < q4) {                                    // uniform
                const f4 w4 = *reinterpret_cast<const f4 *>(&wv[j0]);
                const f4 s4 = *reinterpret_cast<const f4 *>(&sv[j0]);
                a[0] = fmaf(As[j0 * QB + x], w4.x, a[0]);
                a[1] = fmaf(As[(j0 + 1) * QB + x], w4.y, a[1]);
                a[2] = fmaf(As[(j0 + 2) * QB + x], w4.z, a[2]);
                a[3] = fmaf(As[(j0 + 3) * QB + x], w4.w, a[3]);
                grow[j0] = fmaf(coef, s4.x, grow[j0]);        // dA[x][j] += w_t[x] bh_{t+1}[j]
                grow[j0 + 1] = fmaf(coef, s4.y, grow[j0 + 1]);
                grow[j0 + 2] = fmaf(coef, s4.z, grow[j0 + 2]);
                grow[j0 + 3] = fmaf(coef, s4.w, grow[j0 + 3]);
            }
        }
        const float bhbar = (a[0] + a[1]) + (a[2] + a[3]);   // (A^T w_t)[x]
        const float vd[1] = {act ? bhbar * sb : 0.f};
        pgl_publish<1, NW>(vd, r2);
        __syncthreads();
        float d[1];
        pgl_collect<1, NW>(r2, d);
        const float vbar = act ? (bhbar - d[0] * iSb) * iSb : 0.f;
        if (act) dEb[base + (size_t)(t + 1) * q + x] = vbar * rb1;
        float ga, gr;
        pgl_local(G1, al1, rb1, act, mode, s[1], s[2], s[3], &ga, &gr);
        Rbar = ga + vbar * e1;
        rbs = rb1s;
    }
    if (act) {
        float *gp = gpart + ((size_t)row * q + x) * q;
#pragma unroll
        for (int j = 0; j < QB; ++j)
            if (j < q) gp[j] = grow[j];
    }
}

// adjoint of the forward recursion, descending in time: grid k*b, block QB; dynamic LDS At[j][x] = A[x][j]
// (row stride QB).  Writes dEa (d loss / d E' through u), the sequence's dA partial sum_t alpha_hat_{t-1} (x) Rfbar_t
// (row x in lane x) and its dpi.
template <int QB>
__global__ __launch_bounds__(QB) void k_pgl_walk_alpha(const float *__restrict__ A, const float *__restrict__ pi,
                                                       const float *__restrict__ E, const float *__restrict__ AH,
                                                       const float *__restrict__ Sst, const float *__restrict__ RB,
                                                       const float *__restrict__ G, int b, int L, int q, float eps,
                                                       int mode, float *__restrict__ dEa, float *__restrict__ gpart,
                                                       float *__restrict__ dpi_part) {
    extern __shared__ float At[];
    __shared__ __attribute__((aligned(16))) float rv[QB];
    __shared__ float r1[5][2];
    constexpr int NW = QB / 64;
    const long long row = blockIdx.x;
    const int m = (int)(row / b), x = threadIdx.x;
    const int q4 = (q + 3) & ~3;
    const bool act = x < q;
    const float *Am = A + (size_t)m * q * q;
    for (int jj = 0; jj < q4; ++jj) At[jj * QB + x] = (act && jj < q) ? Am[(size_t)x * q + jj] : 0.f;
    const size_t base = (size_t)row * L * q;
    const float *Sr = Sst + (size_t)row * L;
    auto ld = [&](const float *p, int t) { return act ? p[base + (size_t)t * q + x] : 0.f; };
    float grow[QB];
#pragma unroll
    for (int j = 0; j < QB; ++j) grow[j] = 0.f;
    float abar = 0.f;                                         // d loss / d alpha_hat_t from the future
    float ne = ld(E, L - 1), nr = ld(RB, L - 1), na = ld(AH, L - 1), ng = ld(G, L - 1), ns = Sr[L - 1];
    __syncthreads();                                          // At staged
    for (int t = L - 1; t >= 0; --t) {
        const float e = fmaxf(ne, eps), rbs = nr, us = na, Gt = ng, S = ns;
        if (t > 0) { ne = ld(E, t - 1); nr = ld(RB, t - 1); na = ld(AH, t - 1); ng = ld(G, t - 1); ns = Sr[t - 1]; }
        const float u = __builtin_fabsf(us), al = u / S, rb = __builtin_fabsf(rbs);
        const float g = act ? al * rb : 0.f;
        const float v[5] = {g, act ? Gt * g : 0.f, Gt, (act && al > 0.f) ? Gt : 0.f, act ? abar * al : 0.f};
        pgl_publish<5, NW>(v, r1);
        __syncthreads();
        float s[5];
        pgl_collect<5, NW>(r1, s);
        float ga, gr;
        pgl_local(Gt, al, rb, act, mode, s[0], s[1], s[2], &ga, &gr);
        const float dot = s[4] + pgl_gr_dot_al(mode, s[0], s[1], s[2], s[3]);
        const float ubar = act ? (abar + gr - dot) / S : 0.f;
        if (act) dEa[base + (size_t)t * q + x] = ubar * (u / e);              // u_t / E'_t = max(R^f_t, eps)
        const float Rfbar = (act && __builtin_bit_cast(int, us) >= 0) ? ubar * e : 0.f;   // the clamp of R^f_t passes nothing
        if (t > 0) {
            const float alp = __builtin_fabsf(na) / ns;      // alpha_hat_{t-1}[x]
            rv[x] = Rfbar;
            __syncthreads();
            float a[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j0 = 0; j0 < QB; j0 += 4) {
                if (j0 < q4) {                                // uniform
                    const f4 r4 = *reinterpret_cast<const f4 *>(&rv[j0]);
                    a[0] = fmaf(At[j0 * QB + x], r4.x, a[0]);
                    a[1] = fmaf(At[(j0 + 1) * QB + x], r4.y, a[1]);
                    a[2] = fmaf(At[(j0 + 2) * QB + x], r4.z, a[2]);
                    a[3] = fmaf(At[(j0 + 3) * QB + x], r4.w, a[3]);
                    grow[j0] = fmaf(alp, r4.x, grow[j0]);     // dA[x][j] += alpha_hat_{t-1}[x] Rfbar_t[j]
                    grow[j0 + 1] = fmaf(alp, r4.y, grow[j0 + 1]);
                    grow[j0 + 2] = fmaf(alp, r4.z, grow[j0 + 2]);
                    grow[j0 + 3] = fmaf(alp, r4.w, grow[j0 + 3]);
                }
            }
            abar = act ? (a[0] + a[1]) + (a[2] + a[3]) : 0.f;                  // (A Rfbar_t)[x]
        } else if (act) {
            dpi_part[(size_t)row * q + x] = pi[(size_t)m * q + x] > eps ? Rfbar : 0.f;
        }
    }
    if (act) {
        float *gp = gpart + ((size_t)row * q + x) * q;
#pragma unroll
        for (int j = 0; j < QB; ++j)
            if (j < q) gp[j] = grow[j];
    }
}

template <int QB>
static void pgl_walk_launch(const float *A, const float *pi, const float *E, int k, int b, int L, int q, float eps,
                            int mode, const float *G, float *dA, float *dE, const PglLayout &g, char *ws, hipStream_t st) {
    const dim3 grid((unsigned)((size_t)k * b));
    const size_t lds = (size_t)((q + 3) & ~3) * QB * sizeof(float);
    float *AH = (float *)(ws + g.o_ah), *RB = (float *)(ws + g.o_rb), *S = (float *)(ws + g.o_s);
    hipLaunchKernelGGL(k_gl_walk_fwd, grid, dim3(QB), lds, st, A, pi, E, b, L, q, eps, AH, (double *)(ws + g.o_ll), S);
    hipLaunchKernelGGL(k_pgl_walk_rb<QB>, grid, dim3(QB), lds, st, A, E, b, L, q, eps, RB);
    hipLaunchKernelGGL(k_pgl_walk_beta<QB>, grid, dim3(QB), lds, st, A, E, (const float *)AH, (const float *)S,
                       (const float *)RB, G, b, L, q, eps, mode, dE, (float *)(ws + g.o_gpart));
    hipLaunchKernelGGL(k_pgl_walk_alpha<QB>, grid, dim3(QB), lds, st, A, pi, E, (const float *)AH, (const float *)S,
                       (const float *)RB, G, b, L, q, eps, mode, (float *)(ws + g.o_dea), (float *)(ws + g.o_gpart2),
                       (float *)(ws + g.o_dpi));
    hipLaunchKernelGGL(k_pg_grad_sum, dim3(q * q, k), dim3(64), 0, st, (const float *)(ws + g.o_gpart2),
                       (const float *)(ws + g.o_gpart), dA, b, q);
}

// ------------------------------------------------------------------ per-position GEMMs
// deterministic block sums of N values (256 threads), totals broadcast to all
template <int N>
__device__ __forceinline__ void pgl_block_sums(float (&v)[N], float (*red)[4]) {
    const int w = threadIdx.x >> 6;
    __syncthreads();                                          // red free again
#pragma unroll
    for (int x = 0; x < N; ++x) {
        const float s = gl_wave_sum(v[x]);
        if ((threadIdx.x & 63) == 0) red[x][w] = s;
    }
    __syncthreads();
#pragma unroll
    for (int x = 0; x < N; ++x) v[x] = (red[x][0] + red[x][1]) + (red[x][2] + red[x][3]);
}

// the unit operands of the plain-product GEMMs: row sums P[row][0] = 1 (one tile column), log scale 0, E = 1
__global__ __launch_bounds__(256) void k_pgl_unit(float *__restrict__ P, double *__restrict__ ll, float *__restrict__ ones,
                                                  int NB, int q) {
    const size_t x = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (x < (size_t)NB) { P[x * LQ_NTP] = 1.f; ll[x] = 0.0; }
    if (x < (size_t)q) ones[x] = 1.f;
}

// adjoint of the backward recursion at position p (one block per sequence).  BB = A^T w_{p-1} (the plain-product
// GEMM), or null at p = 0.  Writes dEb_p, w_p (masked Rbar_p, the next GEMM's operand) and bh_p (for dA).
__global__ __launch_bounds__(256) void k_pgl_beta_step(const float *__restrict__ E, const float *__restrict__ AH,
                                                       const float *__restrict__ RB, const float *__restrict__ G, int L,
                                                       int q, int p, float eps, int mode, const float *__restrict__ BB,
                                                       float *__restrict__ W, float *__restrict__ BH,
                                                       float *__restrict__ dEb) {
    __shared__ float red[6][4];
    const long long row = blockIdx.x;
    const size_t ot = ((size_t)row * L + p) * q, ov = (size_t)row * q;
    float s[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};             // sum U, U Rb, G U Rb, G, sb, BB sb
    for (int j = threadIdx.x; j < q; j += 256) {
        const float u = __builtin_fabsf(AH[ot + j]), rb = __builtin_fabsf(RB[ot + j]), Gj = G[ot + j];
        s[0] += u; s[1] += u * rb; s[2] += Gj * u * rb; s[3] += Gj;
        if (BB) {
            const float sb = fmaxf(E[ot + j], eps) * rb;
            s[4] += sb; s[5] += BB[ov + j] * sb;
        }
    }
    pgl_block_sums<6>(s, red);
    const float iSu = 1.0f / s[0], Sg = s[1] * iSu, SGg = s[2] * iSu;
    const float iSb = BB ? 1.0f / s[4] : 0.f, dot = s[5] * iSb;
    for (int j = threadIdx.x; j < q; j += 256) {
        const float rbs = RB[ot + j], rb = __builtin_fabsf(rbs), al = __builtin_fabsf(AH[ot + j]) * iSu;
        float ga, gr;
        pgl_local(G[ot + j], al, rb, true, mode, Sg, SGg, s[3], &ga, &gr);
        float Rbar = ga;
        if (BB) {
            const float e = fmaxf(E[ot + j], eps);
            const float vbar = (BB[ov + j] - dot) * iSb;
            dEb[ot + j] = vbar * rb;
            BH[ov + j] = e * rb * iSb;
            Rbar += vbar * e;
        } else {
            dEb[ot + j] = 0.f;                                // bh_0 feeds nothing
        }
        W[ov + j] = __builtin_bit_cast(int, rbs) >= 0 ? Rbar : 0.f;           // the clamp of Rb_p passes nothing
    }
}

// adjoint of the forward recursion at position t (one block per sequence).  AB = A Rfbar_{t+1} (the plain-product
// GEMM), or null at t = L - 1.  Writes dEa_t and, for t > 0, Rfbar_t (the next GEMM's operand) and alpha_hat_{t-1}
// (for dA); at t = 0 the sequence's dpi.
__global__ __launch_bounds__(256) void k_pgl_alpha_step(const float *__restrict__ E, const float *__restrict__ AH,
                                                        const float *__restrict__ RB, const float *__restrict__ G,
                                                        const float *__restrict__ pi, int b, int L, int q, int t,
                                                        float eps, int mode, const float *__restrict__ AB,
                                                        float *__restrict__ RF, float *__restrict__ AP,
                                                        float *__restrict__ dEa, float *__restrict__ dpi_part) {
    __shared__ float red[7][4];
    const long long row = blockIdx.x;
    const int m = (int)(row / b);
    const size_t ot = ((size_t)row * L + t) * q, ov = (size_t)row * q;
    float s[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};        // sum U, U Rb, G U Rb, G, G (U > 0), abar U, U_{t-1}
    for (int j = threadIdx.x; j < q; j += 256) {
        const float u = __builtin_fabsf(AH[ot + j]), rb = __builtin_fabsf(RB[ot + j]), Gj = G[ot + j];
        s[0] += u; s[1] += u * rb; s[2] += Gj * u * rb; s[3] += Gj;
        s[4] += u > 0.f ? Gj : 0.f;
        if (AB) s[5] += AB[ov + j] * u;
        if (t > 0) s[6] += __builtin_fabsf(AH[ot - q + j]);
    }
    pgl_block_sums<7>(s, red);
    const float S = s[0], iS = 1.0f / S, Sg = s[1] * iS, SGg = s[2] * iS;
    const float dot = s[5] * iS + pgl_gr_dot_al(mode, Sg, SGg, s[3], s[4]);
    const float iSp = t > 0 ? 1.0f / s[6] : 0.f;
    for (int j = threadIdx.x; j < q; j += 256) {
        const float us = AH[ot + j], u = __builtin_fabsf(us), al = u * iS, rb = __builtin_fabsf(RB[ot + j]);
        const float e = fmaxf(E[ot + j], eps);
        float ga, gr;
        pgl_local(G[ot + j], al, rb, true, mode, Sg, SGg, s[3], &ga, &gr);
        const float ubar = ((AB ? AB[ov + j] : 0.f) + gr - dot) / S;
        dEa[ot + j] = ubar * (u / e);                                         // u_t / E'_t = max(R^f_t, eps)
        const float Rfbar = __builtin_bit_cast(int, us) >= 0 ? ubar * e : 0.f;  // the clamp of R^f_t passes nothing
        if (t > 0) {
            RF[ov + j] = Rfbar;
            AP[ov + j] = __builtin_fabsf(AH[ot - q + j]) * iSp;
        } else {
            dpi_part[ov + j] = pi[(size_t)m * q + j] > eps ? Rfbar : 0.f;
        }
    }
}

static void pgl_gemm(const float *A, const float *pi, const float *E, int k, int b, int L, int q, float eps, int mode,
                     const float *G, float *dA, float *dE, const PglLayout &g, char *ws, hipStream_t st) {
    const LqPlan &p = g.lq;
    const long long ldt = (long long)L * q;
    const int NB = p.NB;
    float *AH = (float *)(ws + g.o_ah), *RB = (float *)(ws + g.o_rb), *dEa = (float *)(ws + g.o_dea);
    float *P[2] = {(float *)(ws + p.o_P), (float *)(ws + p.o_P) + (size_t)NB * LQ_NTP};
    double *l2[2] = {(double *)(ws + p.o_ll2), (double *)(ws + p.o_ll2) + NB};
    float *X[2] = {(float *)(ws + p.o_X0), (float *)(ws + p.o_X1)};
    float *V[2] = {(float *)(ws + p.o_V0), (float *)(ws + p.o_V1)};
    const float *At = lq_transposed(A, p, ws, st);
    // forward values: signed U_t parked in AH, operands ping-pong in X0 / X1
    {
        hipLaunchKernelGGL(k_lq_init, dim3(NB), dim3(256), 0, st, pi, E, ldt, X[0], (long long)q, (float *)nullptr, 0LL,
                           AH, ldt, 0, P[0], l2[0], q, b, eps);
        int NT = 1;
        for (int t = 1; t < L; ++t) {
            const int i = t & 1;
            LqStep f = {E + (long long)t * q, ldt, P[i ^ 1], P[i], l2[i ^ 1], l2[i], X[i], (long long)q, nullptr, 0,
                        AH + (long long)t * q, ldt, eps, NT, 1};
            lq_gemm(X[i ^ 1], q, At, p, st, f, false, false);
            NT = lq_tile_cols(p);
        }
    }
    // backward values: signed Rb_t parked in RB, operands ping-pong in V0 / V1
    {
        float *Pb[2] = {(float *)(ws + p.o_Pb), (float *)(ws + p.o_Pb) + (size_t)NB * LQ_NTP};
        double *ls[2] = {(double *)(ws + p.o_ls2), (double *)(ws + p.o_ls2) + NB};
        hipLaunchKernelGGL(k_lq_init, dim3(NB), dim3(256), 0, st, (const float *)nullptr, E + (long long)(L - 1) * q, ldt,
                           V[0], (long long)q, (float *)nullptr, 0LL, RB + (long long)(L - 1) * q, ldt, 0, Pb[0], ls[0],
                           q, b, eps);
        int NT = 1;
        for (int t = L - 2; t >= 0; --t) {
            const int i = (L - 1 - t) & 1;
            LqStep f = {E + (long long)t * q, ldt, Pb[i ^ 1], Pb[i], ls[i ^ 1], ls[i], V[i], (long long)q, nullptr, 0,
                        RB + (long long)t * q, ldt, eps, NT, 1};
            lq_gemm(V[i ^ 1], q, A, p, st, f, true, false);
            NT = lq_tile_cols(p);
        }
    }
    // the adjoints: plain products on unit operands (P[0] / l2[0]; P[1] / l2[1] take the unused partials)
    float *ones = (float *)(ws + g.o_ones);
    double *acc = (double *)(ws + g.o_acc);
    const unsigned nu = (unsigned)((std::max(NB, q) + 255) / 256);
    hipLaunchKernelGGL(k_pgl_unit, dim3(nu), dim3(256), 0, st, P[0], l2[0], ones, NB, q);
    (void)hipMemsetAsync(acc, 0, (size_t)k * q * q * sizeof(double), st);
    const int nt = (q + 31) / 32;
    auto product = [&](const float *Xin, const float *Bt, float *out) {
        LqStep f = {ones, 0, P[0], P[1], l2[0], l2[1], out, (long long)q, nullptr, 0, nullptr, 0, -INFINITY, 1, 0};
        lq_gemm(Xin, q, Bt, p, st, f, false, false);
    };
    // adjoint of the backward recursion, ascending: W ping-pong in X0 / X1, bh in V0, A^T w in V1
    float *BH = V[0], *BB = V[1];
    hipLaunchKernelGGL(k_pgl_beta_step, dim3(NB), dim3(256), 0, st, E, (const float *)AH, (const float *)RB, G, L, q, 0,
                       eps, mode, (const float *)nullptr, X[0], (float *)nullptr, dE);
    for (int t = 0; t + 1 < L; ++t) {
        const int i = t & 1;
        product(X[i], At, BB);                                                   // (w_t A)[x] = (A^T w_t)[x]
        hipLaunchKernelGGL(k_pgl_beta_step, dim3(NB), dim3(256), 0, st, E, (const float *)AH, (const float *)RB, G, L, q,
                           t + 1, eps, mode, (const float *)BB, X[i ^ 1], BH, dE);
        hipLaunchKernelGGL(k_gl_dA, dim3(nt, nt, k), dim3(256), 0, st, (const float *)X[i], (const float *)BH, b, q, acc);
    }
    // adjoint of the forward recursion, descending
    float *RF = (float *)(ws + g.o_rf), *AP = (float *)(ws + g.o_ap), *AB = (float *)(ws + g.o_ab);
    float *dpp = (float *)(ws + g.o_dpi);
    for (int t = L - 1; t >= 0; --t) {
        hipLaunchKernelGGL(k_pgl_alpha_step, dim3(NB), dim3(256), 0, st, E, (const float *)AH, (const float *)RB, G, pi, b,
                           L, q, t, eps, mode, t == L - 1 ? (const float *)nullptr : (const float *)AB, RF, AP, dEa, dpp);
        if (t > 0) {
            product(RF, A, AB);                                                  // (Rfbar_t A^T)[x] = (A Rfbar_t)[x]
            hipLaunchKernelGGL(k_gl_dA, dim3(nt, nt, k), dim3(256), 0, st, (const float *)AP, (const float *)RF, b, q, acc);
        }
    }
    const size_t nA = (size_t)k * q * q;
    hipLaunchKernelGGL(k_gl_dA_out, dim3((unsigned)((nA + 255) / 256)), dim3(256), 0, st, (const double *)acc, dA, nA);
}

extern "C" int hmm_posterior_grad_large_max_states(void) { return GL_MAX; }

extern "C" size_t hmm_posterior_grad_large_workspace_bytes(int k, int b, int L, int q) {
    if (k < 1 || b < 1 || L < 1 || q < 1 || q > GL_MAX) return 0;
    PglLayout g;
    pgl_layout(k, b, L, q, &g);
    return g.total;
}

extern "C" int hmm_posterior_grad_large(const float *A, const float *pi, const float *E, int k, int b, int L, int q,
                                        float eps, int mode, const float *grad_out, float *dA, float *dpi, float *dE,
                                        void *workspace, size_t workspace_bytes, void *stream) {
    if (k < 1 || b < 1 || L < 1 || q < 1) return HMM_ERR_BAD_SHAPE;
    if (q > GL_MAX) return HMM_ERR_Q_UNSUPPORTED;
    if (mode != HMM_POST_PROB && mode != HMM_POST_LOG) return HMM_ERR_BAD_ARGUMENT;
    if (!A || !pi || !E || !grad_out || !dA || !dpi || !dE || !workspace) return HMM_ERR_NULL_POINTER;
    if (check_eps(eps)) return HMM_ERR_BAD_ARGUMENT;
    PglLayout g;
    pgl_layout(k, b, L, q, &g);
    if (workspace_bytes < g.total || ((uintptr_t)workspace & 255)) return HMM_ERR_WORKSPACE;
    const int route = opt(HMM_OPT_GLARGE);
    if (route == 1 && q > GL_WALK_MAX) return HMM_ERR_BAD_ARGUMENT;       // never a silent switch of evaluation
    const bool walk = route == 1 || (route != 2 && q <= GL_Q_WALK);
    char *ws = (char *)workspace;
    hipStream_t st = (hipStream_t)stream;
    if (walk) {
        if (q <= 64) pgl_walk_launch<64>(A, pi, E, k, b, L, q, eps, mode, grad_out, dA, dE, g, ws, st);
        else pgl_walk_launch<128>(A, pi, E, k, b, L, q, eps, mode, grad_out, dA, dE, g, ws, st);
    } else {
        pgl_gemm(A, pi, E, k, b, L, q, eps, mode, grad_out, dA, dE, g, ws, st);
    }
    const size_t n = (size_t)k * b * L * q;
    hipLaunchKernelGGL(k_pg_merge, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, E, (const float *)(ws + g.o_dea),
                       dE, n, eps);
    hipLaunchKernelGGL(k_pg_sum_rows, dim3(q, k), dim3(64), 0, st, (const float *)(ws + g.o_dpi), dpi, b, q);
    return check_launch();
}
