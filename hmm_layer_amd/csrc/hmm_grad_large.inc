// hmm_grad_large.inc — gradient of the log-likelihoods for 1 <= q <= 4096 states (hmm_loglik_grad_large),
// included after hmm_midq.inc, hmm_largeq.inc and hmm_grad.inc.
//
// Same derivatives and clamp handling as hmm_grad.inc / k_mq_backward_grad (oracle.textbook.loglik_grad):
//   dE_t = w gamma_t / E_t (0 where E_t <= eps),   dpi = sum_s w gamma_0 / pi (0 where pi <= eps, whatever E_0 is),
//   dA   = sum_t coef_t^T bh_{t+1},  coef_t = alpha_hat_t w / <alpha_hat_t, R_t>,
//   R_t  = max(bh_{t+1} A^T, eps),   bh_t = live_t * normalised(max(E_t, eps) R_t),   gamma_t ∝ alpha_hat_t R_t,
// where live_t[j] says that the forward cell's clamp of the predicted state, (alpha_hat_{t-1} A)[j] <= eps
// (MsaHmmCell.py:88), was not active: a clamped state passes nothing back.  Everything above is scale-free in
// alpha_hat_t, so both evaluations park the UNNORMALISED forward vector U_t = max(E_t, eps) max(R_t, eps) in the
// caller's dE, with the sign bit set where the state was not live, and overwrite it position by position on the
// way back: no workspace grows with L.  bh is normalised before the eps clamp of R (the clamp is not scale-free).
//
// Kernels:
//   k_gl_walk_fwd / k_gl_walk_bwd<QB>   per-sequence walk (HMM_OPT_GLARGE = 1, default for q <= GL_Q_WALK): one
//                 workgroup per sequence, ceil(q/64) waves, lane = state, A (forward) or A^T (backward) in LDS,
//                 the previous vector in LDS.  The forward sweep keeps its previous vector double-buffered with
//                 one barrier per step; the backward sweep needs two cross-wave sums per step (the row sums of
//                 gamma and of the next bh), so it finishes position t + 1 during step t from triple-buffered
//                 vectors — still one barrier per step.  Lane i sums row i of G = sum_t coef_t[i] bh_{t+1}[.] in
//                 registers (fp32 within the sequence); k_mq_grad_sum adds the sequences' G in fp64, fixed order.
//   k_lq_gemm (sign = 1) / k_lq_gemm (backward) + k_gl_bpost + k_gl_dA   per-position GEMMs (HMM_OPT_GLARGE = 2,
//                 default above GL_Q_WALK, valid for every q): the forward recursion of hmm_largeq.inc parks
//                 signed U_t in dE; the adjoint recursion is the backward recursion of hmm_largeq.inc run on the
//                 masked bh (its operand is max(E,eps) R unnormalised, the previous step's partial row sums of the
//                 UNMASKED vector normalise it inside the GEMM before the clamp); k_gl_bpost forms gamma, dE_t and
//                 coef_t and masks the next operand; k_gl_dA adds coef_t^T bh_{t+1} (K = sequences) into an fp64
//                 accumulator, every entry owned by one lane (fixed order).

#define GL_MAX 4096               // hmm_loglik_grad_large_max_states()
#define GL_WALK_MAX 128           // largest q the walk serves (two waves; G row of lane i in registers)
#define GL_Q_WALK 128             // default route: walk for q <= GL_Q_WALK, GEMMs above

struct GlLayout {
    LqPlan lq;                    // the GEMM route's recursions (hmm_largeq.inc), at offset 0
    size_t o_R, o_coef, o_acc, o_ll, o_gpart, total;
};

static void gl_layout(int k, int b, int L, int q, GlLayout *g) {
    make_lqplan(k, b, L, q, &g->lq);
    const size_t nr = (size_t)k * b;
    size_t off = g->lq.total;
    g->o_R = off;     off = align_up(off + nr * q * sizeof(float));              // R_t of the adjoint recursion
    g->o_coef = off;  off = align_up(off + nr * q * sizeof(float));              // coef_t / Sb_{t+1}
    g->o_acc = off;   off = align_up(off + (size_t)k * q * q * sizeof(double));  // dA in fp64
    g->o_ll = off;    off = align_up(off + nr * sizeof(double));
    g->o_gpart = off; off = align_up(off + (q <= GL_WALK_MAX ? nr * q * q * sizeof(float) : 0));   // walk: G per sequence
    g->total = off;
}

__device__ __forceinline__ float gl_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// ------------------------------------------------------------------ per-sequence walk
// forward: grid k*b, block NP = 64 ceil(q/64); dynamic LDS As[i][j] = A[i][j] for i < ceil4(q) (zero padded), row
// stride NP.  Writes signed U_t into dE and the fp64 log-likelihood; Sst (or null) receives the normalisers
// S_t = sum U_t, [row][t] (hmm_posterior_grad_large).
__global__ __launch_bounds__(GL_WALK_MAX) void k_gl_walk_fwd(const float *__restrict__ A, const float *__restrict__ pi,
                                                             const float *__restrict__ E, int b, int L, int q, float eps,
                                                             float *__restrict__ dE, double *__restrict__ ll,
                                                             float *__restrict__ Sst) {
    extern __shared__ float As[];
    __shared__ __attribute__((aligned(16))) float xs[2][GL_WALK_MAX];
    __shared__ float ws[2][2];
    const long long row = blockIdx.x;
    const int m = (int)(row / b), j = threadIdx.x, w = j >> 6, nw = blockDim.x >> 6, NP = blockDim.x;
    const int q4 = (q + 3) & ~3;
    const bool act = j < q;
    const float *Am = A + (size_t)m * q * q;
    for (int i = 0; i < q4; ++i) As[i * NP + j] = (act && i < q) ? Am[(size_t)i * q + j] : 0.f;
    const float *Er = E + (size_t)row * L * q;
    float *o = dE + (size_t)row * L * q;
    double lacc = 0.0;
    float en = act ? Er[j] : 0.f;
    for (int t = 0; t < L; ++t) {
        const float eraw = en;
        if (t + 1 < L && act) en = Er[(size_t)(t + 1) * q + j];
        float R;
        if (t == 0) {
            R = act ? pi[(size_t)m * q + j] : 0.f;
            __syncthreads();                                  // As staged
        } else {
            const int cur = (t - 1) & 1;
            float S = ws[cur][0];
            for (int x = 1; x < nw; ++x) S += ws[cur][x];
            lacc += log((double)S);
            if (Sst && j == 0) Sst[(size_t)row * L + t - 1] = S;
            float a[4] = {0.f, 0.f, 0.f, 0.f};
            for (int i = 0; i < q4; i += 4) {
                const f4 xv = *reinterpret_cast<const f4 *>(&xs[cur][i]);
                a[0] = fmaf(xv.x, As[i * NP + j], a[0]);
                a[1] = fmaf(xv.y, As[(i + 1) * NP + j], a[1]);
                a[2] = fmaf(xv.z, As[(i + 2) * NP + j], a[2]);
                a[3] = fmaf(xv.w, As[(i + 3) * NP + j], a[3]);
            }
            R = ((a[0] + a[1]) + (a[2] + a[3])) / S;
        }
        const float sf = act ? fmaxf(eraw, eps) * fmaxf(R, eps) : 0.f;
        if (act) o[(size_t)t * q + j] = R > eps ? sf : -sf;
        xs[t & 1][j] = sf;
        const float s = gl_wave_sum(sf);
        if ((j & 63) == 0) ws[t & 1][w] = s;
        __syncthreads();
    }
    if (j == 0) {
        const int last = (L - 1) & 1;
        float S = ws[last][0];
        for (int x = 1; x < nw; ++x) S += ws[last][x];
        ll[row] = lacc + log((double)S);
        if (Sst) Sst[(size_t)row * L + L - 1] = S;
    }
}

// backward: grid k*b, block QB (64 or 128); dynamic LDS At[j][i] = A[i][j] for j < ceil4(q), row stride QB.
// Step t forms R_t from bh_{t+1} and publishes g_t = |U_t| R_t and the masked sb_t = max(E_t,eps) R_t with the
// per-wave sums of g_t and of the unmasked sb_t; the same step, with those sums of position t + 1 now visible,
// writes dE_{t+1} and adds coef_{t+1} bh_{t+2} into the G row — the mat-vec and the outer product share one pass.
template <int QB>
__global__ __launch_bounds__(QB) void k_gl_walk_bwd(const float *__restrict__ A, const float *__restrict__ E, int b,
                                                    int L, int q, float eps, const float *__restrict__ gw,
                                                    float *__restrict__ dE, float *__restrict__ gpart) {
    extern __shared__ float At[];
    __shared__ __attribute__((aligned(16))) float sb[3][QB];
    __shared__ float gp[3][2], sp[3][2];
    constexpr int NW = QB / 64;
    const long long row = blockIdx.x;
    const int m = (int)(row / b), i = threadIdx.x, w = i >> 6;
    const int q4 = (q + 3) & ~3;
    const bool act = i < q;
    const float *Am = A + (size_t)m * q * q;
    for (int jj = 0; jj < q4; ++jj) At[jj * QB + i] = (act && jj < q) ? Am[(size_t)i * q + jj] : 0.f;
    for (int x = 0; x < 3; ++x) sb[x][i] = 0.f;               // the slot of position L is read (times 0) at t = L - 2
    const float *Er = E + (size_t)row * L * q;
    float *o = dE + (size_t)row * L * q;
    const float wt = gw ? gw[row] : 1.f;
    float grow[QB];
#pragma unroll
    for (int x = 0; x < QB; ++x) grow[x] = 0.f;
    float gprev = 0.f, eprev = 0.f, alprev = 0.f, ib2 = 0.f;   // position t + 1: g, raw E, |U|; 1 / Sb_{t+2}
    float en = act ? Er[(size_t)(L - 1) * q + i] : 0.f, un = act ? o[(size_t)(L - 1) * q + i] : 0.f;
    auto sum3 = [&](float (*p)[2], int s) {
        float v = p[s][0];
#pragma unroll
        for (int x = 1; x < NW; ++x) v += p[s][x];
        return v;
    };
    // dE of position t1 from its published sums; returns w / Sg.  Position 0 keeps w gamma_0 / eps in its clamped
    // entries for k_mq_grad_pi, which zeroes them.
    auto finish = [&](int t1) {
        const float sc = wt / sum3(gp, t1 % 3);
        if (act) o[(size_t)t1 * q + i] = (eprev > eps || t1 == 0) ? gprev * sc / fmaxf(eprev, eps) : 0.f;
        return sc;
    };
    __syncthreads();                                          // At staged
    for (int t = L - 1; t >= 0; --t) {
        const float eraw = en, us = un;
        if (t > 0 && act) { en = Er[(size_t)(t - 1) * q + i]; un = o[(size_t)(t - 1) * q + i]; }
        float rb = 1.f, ib1 = 0.f;
        if (t < L - 1) {
            ib1 = 1.f / sum3(sp, (t + 1) % 3);
            const float sc = finish(t + 1);
            const bool outer = t < L - 2;                     // position t + 1 has a successor
            const float coef = outer ? alprev * sc * ib2 : 0.f;
            const float *s1 = sb[(t + 1) % 3], *s2 = sb[(t + 2) % 3];
            float a[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j0 = 0; j0 < QB; j0 += 4) {
                if (j0 < q) {                                 // uniform
                    const f4 v1 = *reinterpret_cast<const f4 *>(&s1[j0]);
                    const f4 v2 = *reinterpret_cast<const f4 *>(&s2[j0]);
                    a[0] = fmaf(At[j0 * QB + i], v1.x, a[0]);
                    a[1] = fmaf(At[(j0 + 1) * QB + i], v1.y, a[1]);
                    a[2] = fmaf(At[(j0 + 2) * QB + i], v1.z, a[2]);
                    a[3] = fmaf(At[(j0 + 3) * QB + i], v1.w, a[3]);
                    grow[j0] = fmaf(coef, v2.x, grow[j0]);
                    grow[j0 + 1] = fmaf(coef, v2.y, grow[j0 + 1]);
                    grow[j0 + 2] = fmaf(coef, v2.z, grow[j0 + 2]);
                    grow[j0 + 3] = fmaf(coef, v2.w, grow[j0 + 3]);
                }
            }
            rb = fmaxf(((a[0] + a[1]) + (a[2] + a[3])) * ib1, eps);
        }
        const float al = __builtin_fabsf(us);
        const bool live = __builtin_bit_cast(int, us) >= 0;
        const float g = act ? al * rb : 0.f;
        const float s = act ? fmaxf(eraw, eps) * rb : 0.f;
        sb[t % 3][i] = live ? s : 0.f;
        const float gs = gl_wave_sum(g), ss = gl_wave_sum(s);
        if ((i & 63) == 0) { gp[t % 3][w] = gs; sp[t % 3][w] = ss; }
        gprev = g; eprev = eraw; alprev = al; ib2 = ib1;
        __syncthreads();
    }
    // position 0: its dE and (L > 1) coef_0 bh_1
    const float sc = finish(0);
    if (L > 1) {
        const float coef = alprev * sc * ib2;
        const float *s2 = sb[1];
#pragma unroll
        for (int j0 = 0; j0 < QB; j0 += 4) {
            if (j0 < q) {
                const f4 v2 = *reinterpret_cast<const f4 *>(&s2[j0]);
                grow[j0] = fmaf(coef, v2.x, grow[j0]);
                grow[j0 + 1] = fmaf(coef, v2.y, grow[j0 + 1]);
                grow[j0 + 2] = fmaf(coef, v2.z, grow[j0 + 2]);
                grow[j0 + 3] = fmaf(coef, v2.w, grow[j0 + 3]);
            }
        }
    }
    if (act) {
        float *gpr = gpart + ((size_t)row * q + i) * q;
#pragma unroll
        for (int x = 0; x < QB; ++x)
            if (x < q) gpr[x] = grow[x];
    }
}

// ------------------------------------------------------------------ per-position GEMMs
// after the adjoint GEMM of position t: one block per sequence.  dE_t holds signed U_t, R the GEMM's R_t, nxt its
// next operand max(E_t,eps) R_t (masked here by live_t, in place).  Writes dE_t = w gamma_t / E_t and, when
// coef != null, coef_t / Sb_{t+1} (Sb_{t+1} from the partial row sums that normalised bh_{t+1} in the GEMM, same order).
__global__ __launch_bounds__(256) void k_gl_bpost(const float *__restrict__ E, float *__restrict__ dE,
                                                  const float *__restrict__ R, float *__restrict__ nxt,
                                                  float *__restrict__ coef, const float *__restrict__ Pprev, int NTprev,
                                                  const float *__restrict__ gw, int L, int q, int t, float eps) {
    __shared__ float red[4];
    const long long row = blockIdx.x;
    const size_t ot = ((size_t)row * L + t) * q;
    float *o = dE + ot;
    const float *er = E + ot, *Rr = R + (size_t)row * q;
    float part = 0.f;
    for (int j = threadIdx.x; j < q; j += 256) part += __builtin_fabsf(o[j]) * Rr[j];
    const float Sg = lq_block_sum(part, red);
    const float sc = (gw ? gw[row] : 1.f) / Sg;
    float cb = 0.f;
    if (coef) {
        float S = 0.f;
        for (int u = 0; u < NTprev; ++u) S += Pprev[(size_t)row * LQ_NTP + u];
        cb = sc / S;
    }
    for (int j = threadIdx.x; j < q; j += 256) {
        const float u = o[j], au = __builtin_fabsf(u), e = er[j];
        o[j] = (e > eps || t == 0) ? au * Rr[j] * sc / fmaxf(e, eps) : 0.f;     // (t = 0: as finish(0) of the walk)
        if (coef) coef[(size_t)row * q + j] = au * cb;
        if (__builtin_bit_cast(int, u) < 0) nxt[(size_t)row * q + j] = 0.f;
    }
}

// acc[m] += C^T S over the model's b sequences: C = coef (b x q), S = bh_{t+1} (b x q), both with K = sequence
// outermost.  One workgroup of four waves per 32 x 32 block of acc; wave v takes the groups of four sequences
// 4v, 4v + 16, ... (2 x 2 f32 MFMAs 16x16x4 per group: lane (g, n) supplies C[r + g][i0 + n] and S[r + g][j0 + n],
// accumulator register rr holds (i0 + 4g + rr, j0 + n)).  Four waves per block keep enough loads in flight: at q = 1027,
// b = 1024 one wave per block took 120 us per position (latency-bound), four take 50 us.  The four partials meet in LDS in a fixed
// order (wave 0 + 1 + 2 + 3) and the fp64 addition into acc is by the entry's one owner lane: deterministic.
__global__ __launch_bounds__(256) void k_gl_dA(const float *__restrict__ C, const float *__restrict__ S, int b, int q,
                                               double *__restrict__ acc) {
    __shared__ f4 red[3][4][64];
    const int m = blockIdx.z, i0 = blockIdx.x * 32, j0 = blockIdx.y * 32;
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane >> 4, n = lane & 15;
    const float *Cm = C + (size_t)m * b * q, *Sm = S + (size_t)m * b * q;
    const bool ci0 = i0 + n < q, ci1 = i0 + 16 + n < q, cj0 = j0 + n < q, cj1 = j0 + 16 + n < q;
    f4 d[4];
#pragma unroll
    for (int x = 0; x < 4; ++x) d[x] = (f4){0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int r0 = 4 * wv; r0 < b; r0 += 16) {
        const int r = r0 + g;
        const bool rv = r < b;
        const float *cr = Cm + (size_t)(rv ? r : 0) * q, *sr = Sm + (size_t)(rv ? r : 0) * q;
        const float a0 = (rv && ci0) ? cr[i0 + n] : 0.f, a1 = (rv && ci1) ? cr[i0 + 16 + n] : 0.f;
        const float b0 = (rv && cj0) ? sr[j0 + n] : 0.f, b1 = (rv && cj1) ? sr[j0 + 16 + n] : 0.f;
        d[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, d[0], 0, 0, 0);
        d[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b1, d[1], 0, 0, 0);
        d[2] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b0, d[2], 0, 0, 0);
        d[3] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, d[3], 0, 0, 0);
    }
    if (wv > 0) {
#pragma unroll
        for (int x = 0; x < 4; ++x) red[wv - 1][x][lane] = d[x];
    }
    __syncthreads();
    if (wv != 0) return;
    double *am = acc + (size_t)m * q * q;
#pragma unroll
    for (int x = 0; x < 4; ++x) {
        const f4 v = ((d[x] + red[0][x][lane]) + red[1][x][lane]) + red[2][x][lane];
        const int a = x >> 1, c = x & 1;
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const int ii = i0 + 16 * a + 4 * g + rr, jj = j0 + 16 * c + n;
            if (ii < q && jj < q) am[(size_t)ii * q + jj] += (double)v[rr];
        }
    }
}

__global__ void k_gl_dA_out(const double *__restrict__ acc, float *__restrict__ dA, size_t n) {
    const size_t x = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (x < n) dA[x] = (float)acc[x];
}

static void gl_walk(const float *A, const float *pi, const float *E, int k, int b, int L, int q, float eps,
                    const float *gw, float *dA, float *dE, double *ll, float *gpart, hipStream_t st) {
    const dim3 grid((unsigned)((size_t)k * b));
    const int NP = q <= 64 ? 64 : 128, q4 = (q + 3) & ~3;
    const size_t lds = (size_t)q4 * NP * sizeof(float);
    hipLaunchKernelGGL(k_gl_walk_fwd, grid, dim3(NP), lds, st, A, pi, E, b, L, q, eps, dE, ll, (float *)nullptr);
    if (NP == 64)
        hipLaunchKernelGGL(k_gl_walk_bwd<64>, grid, dim3(64), lds, st, A, E, b, L, q, eps, gw, dE, gpart);
    else
        hipLaunchKernelGGL(k_gl_walk_bwd<128>, grid, dim3(128), lds, st, A, E, b, L, q, eps, gw, dE, gpart);
    hipLaunchKernelGGL(k_mq_grad_sum, dim3(q * q, k), dim3(64), 0, st, (const float *)gpart, dA, b, q);
}

static void gl_gemm(const float *A, const float *pi, const float *E, int k, int b, int L, int q, float eps,
                    const float *gw, float *dA, float *dE, const GlLayout &g, char *ws, hipStream_t st) {
    const LqPlan &p = g.lq;
    const long long ldt = (long long)L * q;
    const int NB = p.NB;
    float *R = (float *)(ws + g.o_R), *coef = (float *)(ws + g.o_coef);
    double *acc = (double *)(ws + g.o_acc), *ll = (double *)(ws + g.o_ll);
    // forward: U_t, signed, parked in dE; operands ping-pong in X0 / X1
    {
        const float *At = lq_transposed(A, p, ws, st);
        float *X[2] = {(float *)(ws + p.o_X0), (float *)(ws + p.o_X1)};
        float *P[2] = {(float *)(ws + p.o_P), (float *)(ws + p.o_P) + (size_t)NB * LQ_NTP};
        double *l2[2] = {(double *)(ws + p.o_ll2), (double *)(ws + p.o_ll2) + NB};
        hipLaunchKernelGGL(k_lq_init, dim3(NB), dim3(256), 0, st, pi, E, ldt, X[0], (long long)q, (float *)nullptr,
                           0LL, dE, ldt, 0, P[0], l2[0], q, b, eps);
        int NT = 1;
        for (int t = 1; t < L; ++t) {
            const int i = t & 1;
            LqStep f = {E + (long long)t * q, ldt, P[i ^ 1], P[i], l2[i ^ 1], l2[i], X[i], (long long)q, nullptr, 0,
                        dE + (long long)t * q, ldt, eps, NT, 1};
            lq_gemm(X[i ^ 1], q, At, p, st, f, false, false);
            NT = lq_tile_cols(p);
        }
        const int last = (L - 1) & 1;
        hipLaunchKernelGGL(k_lq_fwd_finish, dim3((NB + 255) / 256), dim3(256), 0, st, (const float *)P[last],
                           (const double *)l2[last], ll, NB, NT);
    }
    // adjoint recursion: operands (masked max(E,eps) R) ping-pong in V0 / V1
    (void)hipMemsetAsync(acc, 0, (size_t)k * q * q * sizeof(double), st);
    float *V[2] = {(float *)(ws + p.o_V0), (float *)(ws + p.o_V1)};
    float *Pb[2] = {(float *)(ws + p.o_Pb), (float *)(ws + p.o_Pb) + (size_t)NB * LQ_NTP};
    double *ls[2] = {(double *)(ws + p.o_ls2), (double *)(ws + p.o_ls2) + NB};
    hipLaunchKernelGGL(k_lq_init, dim3(NB), dim3(256), 0, st, (const float *)nullptr, E + (long long)(L - 1) * q, ldt,
                       V[0], (long long)q, (float *)nullptr, 0LL, R, (long long)q, 0, Pb[0], ls[0], q, b, eps);
    hipLaunchKernelGGL(k_gl_bpost, dim3(NB), dim3(256), 0, st, E, dE, (const float *)R, V[0], (float *)nullptr,
                       (const float *)Pb[0], 1, gw, L, q, L - 1, eps);
    int NT = 1;
    const int nt = (q + 31) / 32;
    for (int t = L - 2; t >= 0; --t) {
        const int i = (L - 1 - t) & 1;
        LqStep f = {E + (long long)t * q, ldt, Pb[i ^ 1], Pb[i], ls[i ^ 1], ls[i], V[i], (long long)q, nullptr, 0,
                    R, (long long)q, eps, NT, 0};
        lq_gemm(V[i ^ 1], q, A, p, st, f, true, false);
        hipLaunchKernelGGL(k_gl_bpost, dim3(NB), dim3(256), 0, st, E, dE, (const float *)R, V[i], coef,
                           (const float *)Pb[i ^ 1], NT, gw, L, q, t, eps);
        NT = lq_tile_cols(p);
        hipLaunchKernelGGL(k_gl_dA, dim3(nt, nt, k), dim3(256), 0, st, (const float *)coef, (const float *)V[i ^ 1], b, q,
                           acc);
    }
    const size_t nA = (size_t)k * q * q;
    hipLaunchKernelGGL(k_gl_dA_out, dim3((unsigned)((nA + 255) / 256)), dim3(256), 0, st, (const double *)acc, dA, nA);
}

extern "C" int hmm_loglik_grad_large_max_states(void) { return GL_MAX; }

extern "C" size_t hmm_loglik_grad_large_workspace_bytes(int k, int b, int L, int q) {
    if (k < 1 || b < 1 || L < 1 || q < 1 || q > GL_MAX) return 0;
    GlLayout g;
    gl_layout(k, b, L, q, &g);
    return g.total;
}

extern "C" int hmm_loglik_grad_large(const float *A, const float *pi, const float *E, int k, int b, int L, int q,
                                     float eps, const float *grad_loglik, float *dA, float *dpi, float *dE,
                                     double *loglik, void *workspace, size_t workspace_bytes, void *stream) {
    if (k < 1 || b < 1 || L < 1 || q < 1) return HMM_ERR_BAD_SHAPE;
    if (q > GL_MAX) return HMM_ERR_Q_UNSUPPORTED;
    if (!A || !pi || !E || !dA || !dpi || !dE || !workspace) return HMM_ERR_NULL_POINTER;
    if (check_eps(eps)) return HMM_ERR_BAD_ARGUMENT;
    GlLayout g;
    gl_layout(k, b, L, q, &g);
    if (workspace_bytes < g.total || ((uintptr_t)workspace & 255)) return HMM_ERR_WORKSPACE;
    const int route = opt(HMM_OPT_GLARGE);
    if (route == 1 && q > GL_WALK_MAX) return HMM_ERR_BAD_ARGUMENT;       // never a silent switch of evaluation
    const bool walk = route == 1 || (route != 2 && q <= GL_Q_WALK);
    char *ws = (char *)workspace;
    hipStream_t st = (hipStream_t)stream;
    double *ll = (double *)(ws + g.o_ll);
    if (walk)
        gl_walk(A, pi, E, k, b, L, q, eps, grad_loglik, dA, dE, ll, (float *)(ws + g.o_gpart), st);
    else
        gl_gemm(A, pi, E, k, b, L, q, eps, grad_loglik, dA, dE, g, ws, st);
    hipLaunchKernelGGL(k_mq_grad_pi, dim3(q, k), dim3(64), 0, st, pi, E, dE, b, L, q, eps, dpi);
    if (loglik)
        hipLaunchKernelGGL(k_copy_loglik, dim3((k * b + 255) / 256), dim3(256), 0, st, (const double *)ll, loglik, k * b);
    return check_launch();
}
