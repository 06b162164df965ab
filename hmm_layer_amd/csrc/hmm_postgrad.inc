// hmm_postgrad.inc — gradient of a loss on the state POSTERIORS (included by hmm_engine.hip after
// hmm_midq.inc).  The reference differentiates _state_posterior_log_probs_impl by autograd through
// its Python loops (hmm_layer/MsaHMMLayer.py:422-521 with training=True, as its own test script
// does, tests/parallel_rnn_forward.py:70-80); this is the same reverse-mode computation written out.
//
//   forward   R^f_t = t ? alpha_{t-1} A : pi,  u_t = E'_t * max(R^f_t, eps),  alpha_t = u_t / S_t
//   backward  Rb_{L-1} = 1,  Rb_t = max(A bh_{t+1}, eps),  bh_t = E'_t * Rb_t / Sb_t
//   output    g_t = alpha_t * Rb_t,  gamma_t = g_t / Sg_t,  out_t = gamma_t | log gamma_t
// Given G_t = d loss / d out_t:  gbar_t = d loss / d g_t (local), then the adjoint of the backward
// recursion runs FORWARD in time (k_pg_beta) and the adjoint of the forward recursion runs BACKWARD
// (k_pg_alpha); clamps pass nothing (torch.maximum semantics): E' = max(E, eps), max(R^f, eps),
// max(A bh, eps), max(pi, eps).  Four serial sweeps per sequence, lane = state (q <= 64): alpha_hat
// (sign bit = forward clamp active) and S_t from the forward sweep, Rb (sign bit = backward clamp
// active) from the backward sweep, then the two adjoint sweeps, which also accumulate row i of dA in
// lane i.  The sweeps run in pairs, two waves per sequence (k_pg_fb, k_pg_adj).  Training batches are short (L ~ 1e4), where four latency-bound sweeps cost
// ~20 ms; the chunked kernels serve the forward value.

template <int QB>
__device__ __forceinline__ void pg_rb_body(const float *__restrict__ A, const float *__restrict__ E, int b, int L, int q,
                                           float eps, float *__restrict__ RB, const int *__restrict__ need) {
    const int row = blockIdx.x, m = row / b, i = threadIdx.x & 63;
    if (need && !need[row]) return;                          // served by the chunked sweeps (hmm_postgrad_chunked.inc)
    const bool act = i < q;
    const float *Am = A + (size_t)m * q * q;
    float arow[QB];
#pragma unroll
    for (int jj = 0; jj < QB; ++jj) arow[jj] = (act && jj < q) ? Am[(size_t)i * q + jj] : 0.f;
    const float *Er = E + (size_t)row * L * q;
    float *o = RB + (size_t)row * L * q;
    float bh = 0.f;
    const MqRows rows(Er, q, i);
    float en[MQ_PF];
    rows.down(L - 1, 0, en);
    auto step = [&](int t, float eraw) {
        const float e = fmaxf(eraw, eps);
        float rb = 1.f;
        bool live = true;
        if (t < L - 1) {
            const float raw = mq_dense_dot<QB>(arow, bh, i);
            live = raw > eps;
            rb = fmaxf(raw, eps);
        }
        if (act) o[(size_t)t * q + i] = live ? rb : -rb;
        const float sb = act ? e * rb : 0.f;
        bh = sb * __builtin_amdgcn_rcpf(mq_wave_sum(sb));
    };
    mq_drain();
    int tb = L - 1;
    for (; tb - MQ_PF + 1 >= 0; tb -= MQ_PF) {              // whole blocks: no branch inside (hmm_midq.inc, MqRows)
        float ce[MQ_PF];
#pragma unroll
        for (int u = 0; u < MQ_PF; ++u) ce[u] = en[u];
        rows.down(tb - MQ_PF, 0, en);
#pragma unroll
        for (int u = 0; u < MQ_PF; ++u) step(tb - u, ce[u]);
    }
#pragma unroll
    for (int u = 0; u < MQ_PF; ++u)
        if (tb - u >= 0) step(tb - u, en[u]);               // wave-uniform
}

// The local adjoint gbar_t = d loss / d g_t (g = alpha * Rb) is only ever used as gbar * alpha
// (-> R-bar) and gbar * Rb (-> alpha-bar); both products are formed directly, so the log mode never
// divides by a posterior that underflowed (G / g would overflow where G / Rb and G / alpha do not).
//   mode 0, out = gamma:      gbar = (G - <G, gamma>) / Sg
//   mode 1, out = log gamma:  gbar = G / g - sum(G) / Sg
__device__ __forceinline__ void pg_local(float G, float al, float rb, bool act, int mode, float *ga, float *gr,
                                         float *inv_sg = nullptr, float *gamma = nullptr) {
    const float g = act ? al * rb : 0.f;
    const float ig = __builtin_amdgcn_rcpf(mq_wave_sum(g));
    if (inv_sg) *inv_sg = ig;
    if (gamma) *gamma = g * ig;
    if (mode == 0) {
        const float dot = mq_wave_sum(act ? G * g * ig : 0.f);
        const float gb = act ? (G - dot) * ig : 0.f;
        *ga = gb * al;
        *gr = gb * rb;
    } else {
        const float c = mq_wave_sum(act ? G : 0.f) * ig;
        *ga = act ? (rb > 0.f ? G / rb : 0.f) - c * al : 0.f;
        *gr = act ? (al > 0.f ? G / al : 0.f) - c * rb : 0.f;
    }
}

// Where a state reads its upstream gradient: the G loader of every adjoint sweep (here and in
// hmm_postgrad_chunked.inc).  PgStateG: G is (k,b,L,q) and state x of position t reads G[t][x] — hmm_posterior_grad.
// PgClassG: G is (k,b,L,C) and a state reads its CLASS's entry, G[t][class(x)], in place — hmm_class_posterior_grad
// (hmm_class_posterior.inc); the table travels by value, four bits per state.
//   seq(row, L, q)  row 0 of sequence `row`;  stride(q)  floats per position;  col(x)  state x's entry within a position
struct PgStateG {
    const float *G;
    __device__ __forceinline__ const float *seq(size_t row, int L, int q) const { return G + row * L * q; }
    __device__ __forceinline__ int stride(int q) const { return q; }
    __device__ __forceinline__ int col(int x) const { return x; }
};
struct PgClassG {
    const float *G;
    unsigned long long cls;                       // class of state s in bits 4 s .. 4 s + 3 (q <= 16)
    int C;
    __device__ __forceinline__ const float *seq(size_t row, int L, int) const { return G + row * L * C; }
    __device__ __forceinline__ int stride(int) const { return C; }
    __device__ __forceinline__ int col(int x) const { return (int)(cls >> (4 * (x & 15))) & 15; }
};

struct PgSide {
    float inv_sg, g_over_gamma, g_tiny, g_all;    // sum 1 / Sg_t;  sum |G| / gamma over gamma >= PG_TINY_GAMMA;  sum |G| below it;  sum |G|
    float zman;                                   // product of the steps' normalisers = zman * 2^zexp
    int zexp;
};
#define PG_TINY_GAMMA 1e-8f

// adjoint of the backward recursion, ascending in time.  dEb[t] receives d loss / d E'_t through bh_t.
// The sweep covers the steps t -> t+1 for t in [t0, t1) of sequence `row` (the whole sequence: 0, L), entered
// with Rbar_in = d loss / d Rb_{t0} (0 for t0 = 0: position 0 has only its own output term) and leaves
// d loss / d Rb_{t1} in *Rbar_out.  ACC: store dEb and the sweep's part of dA (row x of it in lane x: gp[i]).
// side (or null): the product of the normalisers Sb_{t+1} of the steps, as zman * 2^zexp.
template <int QB, bool ACC, class GL = PgStateG>
__device__ __forceinline__ void pg_beta_body(const float *__restrict__ A, const float *__restrict__ E,
                                             const float *__restrict__ AH, const float *__restrict__ RB,
                                             const GL G, int row, int m, int L, int q, float eps, int mode,
                                             int t0, int t1, float Rbar_in, float *Rbar_out, PgSide *side,
                                             float *__restrict__ dEb, float *__restrict__ gp) {
    const int x = threadIdx.x & 63;
    const bool act = x < q;
    const float *Am = A + (size_t)m * q * q;
    float acol[QB], grow[QB];
#pragma unroll
    for (int i = 0; i < QB; ++i) { acol[i] = (act && i < q) ? Am[(size_t)i * q + x] : 0.f; grow[i] = 0.f; }
    const size_t base = (size_t)row * L * q;
    auto ld = [&](const float *p, int t) { return (act && t < L) ? p[base + (size_t)t * q + x] : 0.f; };
    const float *Gs = G.seq((size_t)row, L, q);
    const int gq = G.stride(q), gx = G.col(x);
    float rbs = ld(RB, t0);
    float Rbar = Rbar_in;
    if (t0 == 0) {                                           // R-bar of position 0: only the output term
        float unused;
        pg_local(act ? Gs[gx] : 0.f, __builtin_fabsf(ld(AH, 0)), __builtin_fabsf(rbs), act, mode, &Rbar, &unused);
        if (ACC && act) dEb[base + x] = 0.f;                 // bh_0 feeds nothing
    }
    // the rows of position t + 1 for the steps t = t0 .. tend - 1, MQ_PF steps ahead and with no branch around the
    // loads (MqRows, hmm_midq.inc: with one row in flight the wave slept a memory latency per step)
    const int tend = min(t1, L - 1);
    const MqRows rE(E + base, q, x), rR(RB + base, q, x), rA(AH + base, q, x), rG(Gs, gq, gx);
    float ne[MQ_PF], nr[MQ_PF], na[MQ_PF], ng[MQ_PF];
    rE.up(t0 + 1, tend + 1, ne); rR.up(t0 + 1, tend + 1, nr); rA.up(t0 + 1, tend + 1, na); rG.up(t0 + 1, tend + 1, ng);
    float zm = 1.f;
    int ze = 0;
    auto step = [&](int t, float e1raw, float rb1s, float al1s, float G1) {
        const float e1 = fmaxf(e1raw, eps), al1 = __builtin_fabsf(al1s);
        const float rb1 = __builtin_fabsf(rb1s);
        const float w = (act && __builtin_bit_cast(int, rbs) >= 0) ? Rbar : 0.f;      // clamp of Rb_t passes nothing
        const float sb = act ? e1 * rb1 : 0.f;
        const float Sb = mq_wave_sum(sb);
        const float iSb = __builtin_amdgcn_rcpf(Sb);
        if (side) {
            zm *= Sb;
            ze += __builtin_amdgcn_frexp_expf(zm);
            zm = __builtin_amdgcn_frexp_mantf(zm);
        }
        const float bh1 = sb * iSb;
        MqDense<QB> dw;
        dw.spread(w, x);
        float r4[4] = {0.f, 0.f, 0.f, 0.f};
        MqDenseLoop<QB, 0>::dot(dw, acol, r4);                                    // bhbar[x] = sum_i A[i][x] w[i]
        if (ACC) {
            MqDense<QB> db;
            db.spread(bh1, x);
            MqDenseLoop<QB, 0>::outer(db, w, grow);                               // dA[x][i] += w[x] bh_{t+1}[i]
        }
        const float bhbar = (r4[0] + r4[1]) + (r4[2] + r4[3]);
        const float dot = mq_wave_sum(act ? bhbar * bh1 : 0.f);
        const float vbar = act ? (bhbar - dot) * iSb : 0.f;
        if (ACC && act) dEb[base + (size_t)(t + 1) * q + x] = vbar * rb1;
        float ga, gr;
        pg_local(G1, al1, rb1, act, mode, &ga, &gr);
        Rbar = ga + vbar * e1;
        rbs = rb1s;
    };
    mq_drain();
    int tb = t0;
    for (; tb + MQ_PF <= tend; tb += MQ_PF) {
        float ce[MQ_PF], cr[MQ_PF], ca[MQ_PF], cg[MQ_PF];
#pragma unroll
        for (int u = 0; u < MQ_PF; ++u) { ce[u] = ne[u]; cr[u] = nr[u]; ca[u] = na[u]; cg[u] = ng[u]; }
        const int nt = tb + MQ_PF + 1;
        rE.up(nt, tend + 1, ne); rR.up(nt, tend + 1, nr); rA.up(nt, tend + 1, na); rG.up(nt, tend + 1, ng);
#pragma unroll
        for (int u = 0; u < MQ_PF; ++u) step(tb + u, ce[u], cr[u], ca[u], cg[u]);
    }
#pragma unroll
    for (int u = 0; u < MQ_PF; ++u)
        if (tb + u < tend) step(tb + u, ne[u], nr[u], na[u], ng[u]);              // wave-uniform
    *Rbar_out = Rbar;
    if (side) { side->zman = zm; side->zexp = ze; }
    if (ACC && act) {
#pragma unroll
        for (int i = 0; i < QB; ++i)
            if (i < q) gp[i] = grow[i];
    }
}

// adjoint of the forward recursion, descending in time: dEa[t] = d loss / d E'_t through alpha_t, its own
// partial of dA, and dpi (per sequence).  The sweep covers positions t1-1 .. t0 of sequence `row` (the whole
// sequence: 0, L), entered with abar_in = d loss / d alpha_{t1-1} from the future (0 for t1 = L) and leaves
// d loss / d alpha_{t0-1} in *abar_out.  side (or null; the same values in every lane): what the chunked path
// needs to know about these positions — the routing sums (hmm_postgrad_chunked.inc) and the product of the
// normalisers S_t as zman * 2^zexp.
template <int QB, bool ACC, class GL = PgStateG>
__device__ __forceinline__ void pg_alpha_body(const float *__restrict__ A, const float *__restrict__ pi,
                                              const float *__restrict__ E, const float *__restrict__ AH,
                                              const float *__restrict__ Sst, const float *__restrict__ RB,
                                              const GL G, int row, int m, int L, int q, float eps, int mode,
                                              int t0, int t1, float abar_in, float *abar_out, PgSide *side,
                                              float *__restrict__ dEa, float *__restrict__ gp,
                                              float *__restrict__ dpi_part) {
    const int x = threadIdx.x & 63;
    const bool act = x < q;
    const float *Am = A + (size_t)m * q * q;
    float arow[QB], grow[QB];
#pragma unroll
    for (int j = 0; j < QB; ++j) {
        arow[j] = (act && j < q) ? Am[(size_t)x * q + j] : 0.f;
        grow[j] = 0.f;
    }
    const size_t base = (size_t)row * L * q;
    auto ld = [&](const float *p, int t) { return (act && t >= 0) ? p[base + (size_t)t * q + x] : 0.f; };
    float abar = abar_in;                                    // d loss / d alpha_t from the future
    // rows t1 - 1 .. t0 (alpha_hat one further: the step at t also reads alpha_hat_{t-1}), MQ_PF steps ahead, no branch
    // around the loads; the normalisers S_t come the same way (one value per row, every lane reads it)
    const int alo = max(t0 - 1, 0);
    const MqRows rE(E + base, q, x), rR(RB + base, q, x), rA(AH + base, q, x), rG(G.seq((size_t)row, L, q), G.stride(q), G.col(x)),
        rS(Sst + (size_t)row * L, 1, 0);
    float ne[MQ_PF], nr[MQ_PF], na[MQ_PF], ng[MQ_PF], ns[MQ_PF];
    rE.down(t1 - 1, t0, ne); rR.down(t1 - 1, t0, nr); rA.down(t1 - 1, alo, na); rG.down(t1 - 1, t0, ng); rS.down(t1 - 1, t0, ns);
    float phis = 0.f, c_p = 0.f, c_q = 0.f, c_t = 0.f, zm = 1.f;
    int ze = 0;
    auto step = [&](int t, float eraw, float ahs, float rbs_, float Gt, float S, float ahprev) {
        const float e = fmaxf(eraw, eps), rb = __builtin_fabsf(rbs_);
        const float al = __builtin_fabsf(ahs);
        float ga, gr, isg, gam;
        pg_local(Gt, al, rb, act, mode, &ga, &gr, &isg, &gam);
        if (side) {
            zm *= S;
            ze += __builtin_amdgcn_frexp_expf(zm);
            zm = __builtin_amdgcn_frexp_mantf(zm);
            phis += isg;
            const float w = act ? __builtin_fabsf(Gt) : 0.f;
            const bool tiny = !(gam >= PG_TINY_GAMMA);
            c_t += w;
            c_q += tiny ? w : 0.f;
            c_p += tiny ? 0.f : w * __builtin_amdgcn_rcpf(gam);
        }
        const float ab = abar + gr;
        const float dot = mq_wave_sum(act ? ab * al : 0.f);
        const float ubar = act ? (ab - dot) * __builtin_amdgcn_rcpf(S) : 0.f;
        const float Rf = al * S * __builtin_amdgcn_rcpf(e);                       // max(R^f_t, eps) = u_t / E'_t
        if (ACC && act) dEa[base + (size_t)t * q + x] = ubar * Rf;
        const float Rfbar = (act && __builtin_bit_cast(int, ahs) >= 0) ? ubar * e : 0.f;   // clamp of R^f_t passes nothing
        if (t > 0) {
            const float alp = __builtin_fabsf(ahprev);                            // alpha_hat_{t-1}[x]
            MqDense<QB> dr;
            dr.spread(Rfbar, x);
            float r4[4] = {0.f, 0.f, 0.f, 0.f};
            MqDenseLoop<QB, 0>::dot(dr, arow, r4);                                // abar_{t-1}[x] = sum_j A[x][j] Rfbar[j]
            if (ACC) MqDenseLoop<QB, 0>::outer(dr, alp, grow);                    // dA[x][j] += alpha_{t-1}[x] Rfbar[j]
            abar = (r4[0] + r4[1]) + (r4[2] + r4[3]);
        } else {
            if (ACC && act) dpi_part[(size_t)row * q + x] = pi[(size_t)m * q + x] > eps ? Rfbar : 0.f;
            abar = 0.f;
        }
    };
    mq_drain();
    int tb = t1 - 1;
    for (; tb - MQ_PF + 1 >= t0; tb -= MQ_PF) {
        float ce[MQ_PF], cr[MQ_PF], ca[MQ_PF], cg[MQ_PF], cs[MQ_PF];
#pragma unroll
        for (int u = 0; u < MQ_PF; ++u) { ce[u] = ne[u]; cr[u] = nr[u]; ca[u] = na[u]; cg[u] = ng[u]; cs[u] = ns[u]; }
        const int nt = tb - MQ_PF;
        rE.down(nt, t0, ne); rR.down(nt, t0, nr); rA.down(nt, alo, na); rG.down(nt, t0, ng); rS.down(nt, t0, ns);
#pragma unroll
        for (int u = 0; u < MQ_PF; ++u)
            step(tb - u, ce[u], ca[u], cr[u], cg[u], cs[u], u + 1 < MQ_PF ? ca[u + 1] : na[0]);
    }
#pragma unroll
    for (int u = 0; u < MQ_PF; ++u)
        if (tb - u >= t0)                                                         // wave-uniform
            step(tb - u, ne[u], na[u], nr[u], ng[u], ns[u], u + 1 < MQ_PF ? na[u + 1] : 0.f);
    *abar_out = abar;
    if (side) {
        side->inv_sg = phis;
        side->g_over_gamma = mq_wave_sum(c_p);
        side->g_tiny = mq_wave_sum(c_q);
        side->g_all = mq_wave_sum(c_t);
        side->zman = zm;
        side->zexp = ze;
    }
    if (ACC && act) {
#pragma unroll
        for (int j = 0; j < QB; ++j)
            if (j < q) gp[j] = grow[j];
    }
}

// The four sweeps pair up: forward || backward, then the two adjoint sweeps || each other — wave 0 and
// wave 1 of one workgroup per sequence (they are latency-bound dependent chains; side by side they
// cost one sweep each, 22 -> 12 ms at b = 32 x L = 9999).
template <int QB>
__global__ __launch_bounds__(128) void k_pg_fb(const float *__restrict__ A, const float *__restrict__ pi,
                                               const float *__restrict__ E, int b, int L, int q, float eps,
                                               float *__restrict__ AH, double *__restrict__ ll, float *__restrict__ S,
                                               float *__restrict__ RB, const int *__restrict__ need) {
    if (__builtin_amdgcn_readfirstlane(threadIdx.x >> 6) == 0)
        mq_forward_body<QB, true>(A, pi, E, b, L, q, eps, AH, nullptr, ll, S, need);
    else
        pg_rb_body<QB>(A, E, b, L, q, eps, RB, need);
}

template <int QB, class GL = PgStateG>
__global__ __launch_bounds__(128) void k_pg_adj(const float *__restrict__ A, const float *__restrict__ pi,
                                                const float *__restrict__ E, const float *__restrict__ AH,
                                                const float *__restrict__ S, const float *__restrict__ RB,
                                                const GL G, int b, int L, int q, float eps, int mode,
                                                float *__restrict__ dEb, float *__restrict__ dEa,
                                                float *__restrict__ gpart_b, float *__restrict__ gpart_a,
                                                float *__restrict__ dpi_part, const int *__restrict__ need) {
    const int row = blockIdx.x, m = row / b, x = threadIdx.x & 63;
    if (need && !need[row]) return;                          // served by the chunked sweeps (hmm_postgrad_chunked.inc)
    float leaves;
    if (__builtin_amdgcn_readfirstlane(threadIdx.x >> 6) == 0)
        pg_beta_body<QB, true>(A, E, AH, RB, G, row, m, L, q, eps, mode, 0, L, 0.f, &leaves, nullptr, dEb,
                               gpart_b + ((size_t)row * q + x) * q);
    else
        pg_alpha_body<QB, true>(A, pi, E, AH, S, RB, G, row, m, L, q, eps, mode, 0, L, 0.f, &leaves, nullptr, dEa,
                                gpart_a + ((size_t)row * q + x) * q, dpi_part);
}

// dE = the two contributions to d loss / d E', where the cell did not clamp E
__global__ __launch_bounds__(256) void k_pg_merge(const float *__restrict__ E, const float *__restrict__ dEa,
                                                  float *__restrict__ dE, size_t n, float eps) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dE[i] = E[i] > eps ? dE[i] + dEa[i] : 0.f;
}

// sum of 64 lane partials in a fixed order (fp64 butterfly: the same tree for every call)
__device__ __forceinline__ double pg_wave_sum_d(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// dA[m][e] = sum over the model's sequences of both per-sequence partials, fp64, fixed order: one wave per entry,
// lane s takes sequences s, s + 64, ... (a single thread per entry walking all b sequences took 0.45 ms at
// b = 1024, a tenth of the whole call)
__global__ __launch_bounds__(64) void k_pg_grad_sum(const float *__restrict__ ga, const float *__restrict__ gb,
                                                    float *__restrict__ dA, int b, int q) {
    const int m = blockIdx.y, e = blockIdx.x;
    const size_t o = (size_t)m * b * q * q + e;
    double acc = 0.0;
    for (int r = threadIdx.x; r < b; r += 64) acc += (double)gb[o + (size_t)r * q * q] + (double)ga[o + (size_t)r * q * q];
    acc = pg_wave_sum_d(acc);
    if (threadIdx.x == 0) dA[(size_t)m * q * q + e] = (float)acc;
}

// dpi[m][j] = sum over the model's sequences, the same way
__global__ __launch_bounds__(64) void k_pg_sum_rows(const float *__restrict__ part, float *__restrict__ out, int b, int q) {
    const int m = blockIdx.y, j = blockIdx.x;
    double acc = 0.0;
    for (int r = threadIdx.x; r < b; r += 64) acc += (double)part[((size_t)m * b + r) * q + j];
    acc = pg_wave_sum_d(acc);
    if (threadIdx.x == 0) out[(size_t)m * q + j] = (float)acc;
}

struct PgPlan { size_t o_ah, o_rb, o_dea, o_s, o_ll, o_gpart, o_gpart2, o_dpi, total; };
static void make_pgplan(int k, int b, int L, int q, PgPlan *p) {
    const size_t nb = (size_t)k * b;
    size_t off = 0;
    p->o_ah = off;     off = align_up(off + nb * L * q * sizeof(float));
    p->o_rb = off;     off = align_up(off + nb * L * q * sizeof(float));
    p->o_dea = off;    off = align_up(off + nb * L * q * sizeof(float));
    p->o_s = off;      off = align_up(off + nb * L * sizeof(float));
    p->o_ll = off;     off = align_up(off + nb * sizeof(double));
    p->o_gpart = off;  off = align_up(off + nb * q * q * sizeof(float));
    p->o_gpart2 = off; off = align_up(off + nb * q * q * sizeof(float));
    p->o_dpi = off;    off = align_up(off + nb * q * sizeof(float));
    p->total = off;
}

template <int QB, class GL>
static void pg_launch(const float *A, const float *pi, const float *E, int k, int b, int L, int q, float eps, int mode,
                      const GL G, float *dA, float *dE, char *ws, const PgPlan &pp, hipStream_t st,
                      const int *need = nullptr) {
    const dim3 grid((unsigned)(k * b));
    float *AH = (float *)(ws + pp.o_ah), *RB = (float *)(ws + pp.o_rb), *S = (float *)(ws + pp.o_s);
    float *dEa = (float *)(ws + pp.o_dea);
    float *gb = (float *)(ws + pp.o_gpart), *ga = (float *)(ws + pp.o_gpart2), *dpp = (float *)(ws + pp.o_dpi);
    hipLaunchKernelGGL((k_pg_fb<QB>), grid, dim3(128), 0, st, A, pi, E, b, L, q, eps, AH, (double *)(ws + pp.o_ll), S, RB, need);
    hipLaunchKernelGGL((k_pg_adj<QB, GL>), grid, dim3(128), 0, st, A, pi, E, (const float *)AH, (const float *)S,
                       (const float *)RB, G, b, L, q, eps, mode, dE, dEa, gb, ga, dpp, need);
    const size_t n = (size_t)k * b * L * q;
    hipLaunchKernelGGL(k_pg_merge, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, E, (const float *)dEa, dE, n, eps);
    hipLaunchKernelGGL(k_pg_grad_sum, dim3(q * q, k), dim3(64), 0, st, (const float *)ga, (const float *)gb, dA, b, q);
}

#include "hmm_postgrad_chunked.inc"

extern "C" {

int hmm_posterior_grad_max_states(void) { return MQ_MAX; }

size_t hmm_posterior_grad_workspace_bytes(int k, int b, int L, int q) {
    if (k < 1 || b < 1 || L < 1 || q < 1 || q > MQ_MAX) return 0;
    if (pc_wanted(k, b, L, q)) {
        PcPlan pc;
        return make_pcplan(k, b, L, q, &pc) ? 0 : pc.total;
    }
    PgPlan pp;
    make_pgplan(k, b, L, q, &pp);
    return pp.total;
}

int hmm_posterior_grad(const float *A, const float *pi, const float *E, int k, int b, int L, int q, float eps,
                       int mode, const float *grad_out, float *dA, float *dpi, float *dE,
                       void *workspace, size_t workspace_bytes, void *stream) {
    if (k < 1 || b < 1 || L < 1 || q < 1) return HMM_ERR_BAD_SHAPE;
    if (q > MQ_MAX) return HMM_ERR_Q_UNSUPPORTED;
    if (mode != HMM_POST_PROB && mode != HMM_POST_LOG) return HMM_ERR_BAD_ARGUMENT;
    if (!A || !pi || !E || !grad_out || !dA || !dpi || !dE || !workspace) return HMM_ERR_NULL_POINTER;
    if (check_eps(eps)) return HMM_ERR_BAD_ARGUMENT;
    char *ws = (char *)workspace;
    hipStream_t st = (hipStream_t)stream;
    if (q == 1) {
        // gamma = 1 identically, whatever A, pi and E: every gradient is exactly zero.  The sweeps return rounding
        // noise instead: alpha_hat = sf * v_rcp_f32(sf) is 1 only to an ulp, the centring terms G (1 - alpha_hat) do
        // not cancel, and over b * L positions dA collects 1e-6 per unit of |G| (measured: 1.08e-6 at b = 3, L = 203).
        PgPlan pp;
        make_pgplan(k, b, L, q, &pp);
        if (workspace_bytes < pp.total || ((uintptr_t)workspace & 255)) return HMM_ERR_WORKSPACE;
        if (hipMemsetAsync(dA, 0, (size_t)k * sizeof(float), st) != hipSuccess ||
            hipMemsetAsync(dpi, 0, (size_t)k * sizeof(float), st) != hipSuccess ||
            hipMemsetAsync(dE, 0, (size_t)k * b * L * sizeof(float), st) != hipSuccess)
            return HMM_ERR_LAUNCH;
        return HMM_OK;
    }
    if (pc_wanted(k, b, L, q)) {
        PcPlan pc;
        int rc = make_pcplan(k, b, L, q, &pc);
        if (rc) return rc;
        if (workspace_bytes < pc.total || ((uintptr_t)workspace & 255)) return HMM_ERR_WORKSPACE;
        return pc_launch(A, pi, E, k, b, L, q, eps, mode, PgStateG{grad_out}, dA, dpi, dE, ws, pc, st);
    }
    PgPlan pp;
    make_pgplan(k, b, L, q, &pp);
    if (workspace_bytes < pp.total || ((uintptr_t)workspace & 255)) return HMM_ERR_WORKSPACE;
    if (q <= 16) pg_launch<16>(A, pi, E, k, b, L, q, eps, mode, PgStateG{grad_out}, dA, dE, ws, pp, st);
    else if (q <= 32) pg_launch<32>(A, pi, E, k, b, L, q, eps, mode, PgStateG{grad_out}, dA, dE, ws, pp, st);
    else if (q <= 48) pg_launch<48>(A, pi, E, k, b, L, q, eps, mode, PgStateG{grad_out}, dA, dE, ws, pp, st);
    else pg_launch<64>(A, pi, E, k, b, L, q, eps, mode, PgStateG{grad_out}, dA, dE, ws, pp, st);
    hipLaunchKernelGGL(k_pg_sum_rows, dim3(q, k), dim3(64), 0, st, (const float *)(ws + pp.o_dpi), dpi, b, q);
    return check_launch();
}

long long hmm_posterior_grad_serial_count(int k, int b, int L, int q, const void *workspace, size_t workspace_bytes) {
    if (k < 1 || b < 1 || L < 1 || q < 1 || q > MQ_MAX) return HMM_ERR_BAD_SHAPE;
    if (!pc_wanted(k, b, L, q)) return (long long)k * b;     // the serial sweeps served every sequence
    PcPlan pc;
    int rc = make_pcplan(k, b, L, q, &pc);
    if (rc) return rc;
    if (!workspace) return HMM_ERR_NULL_POINTER;
    if (workspace_bytes < pc.total) return HMM_ERR_WORKSPACE;
    std::vector<int> need((size_t)pc.p.NB);
    if (hipMemcpy(need.data(), (const char *)workspace + pc.o_need, need.size() * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess)
        return HMM_ERR_LAUNCH;
    long long n = 0;
    for (int v : need) n += v != 0;
    return n;
}

}  // extern "C"
