// hmm_postgradwq.inc — gradient of a loss on the state posteriors for 65 <= q <= 256 states by a per-sequence walk with
// the sparse step (hmm_posterior_grad_walk), included by hmm_engine.hip after hmm_postgrad_large.inc.
//
// The derivatives, modes and clamp handling are those stated at the top of hmm_postgrad_large.inc, and so are the four
// sweeps; what differs is the step: the lists, hub columns and verdict of k_wq_prep (hmm_wideq.inc, called with
// force_dense = 0: HMM_OPT_FORCE_DENSE does not act here).  One workgroup per sequence, NP = 64 ceil(q/64) threads,
// lane = state, <= 8 (index, weight) pairs per lane in registers, gathers from an LDS vector; a hub's sum is the
// workgroup-wide sum of the lanes' entries into / out of the hub, wave sums published before a barrier and added in
// wave order by every lane after it.
//
//   1  k_gw_fwd<true>   (hmm_gradwq.inc, unchanged) signed U_t into the workspace.  S_t = sum |U_t| is not stored: the
//                       adjoints form it again from the stored |U_t| with the same wave-sum order.
//   2  k_pgw_rb         signed Rb_t into the workspace, descending, one barrier per step; gather over the successors
//                       (bsrc / bw), hubs through hout.
//   3  k_pgw_beta       adjoint of the backward recursion, ascending.  bhbar = A^T w_t is a gather of w at the
//                       predecessors (fsrc / fw), a hub's is sum_i hin[h][i] w_t[i].  Writes its share of dE into the
//                       caller's dE.
//   4  k_pgw_alpha      adjoint of the forward recursion, descending.  abar = A Rfbar_t is a gather of Rfbar at the
//                       successors (bsrc / bw), a hub's is sum_j hout[h][j] Rfbar_t[j].  Reads the element of dE that
//                       sweep 3 left, adds its own, applies the E > eps mask and writes it back; dpi per sequence at
//                       t = 0.
// Each adjoint step has two barriers (the normalisation adjoint's dot product depends on the step's own mat-vec).
// Rings of PGW_PF rows are in flight for everything read per position.  The four sweeps are four launches of one
// group each: a sweep reads what the one before stored for ALL positions, so pairing two of them in one workgroup
// (hmm_wideq.inc's layout) would only pair the value sweeps or the adjoints among themselves and would double the
// registers a workgroup holds; with one group each, four workgroups of four waves share a CU.
//
// dA on the support of A.  Each adjoint has its own owner per edge — the operands its mat-vec has just gathered:
//   sweep 3  dA[i][j] += w_t[i] bh_{t+1}[j]: destination lane j, slot e of its predecessor list (the gathered
//            w_t[fsrc[j][e]] times its own bh_{t+1}[j]); edges INTO a hub h: source lane i, from the published
//            bh_{t+1}[h].
//   sweep 4  dA[i][j] += alpha_hat_{t-1}[i] Rfbar_t[j]: source lane i, slot e of its successor list (the gathered
//            Rfbar_t[bsrc[i][e]] times its own alpha_hat_{t-1}[i]); edges OUT OF a hub h: destination lane j, from the
//            published alpha_hat_{t-1}[h].  alpha_hat_{t-1} needs S_{t-1}, which step t - 1 forms: the products of
//            position t are added one step later, from registers.
// That is GW_ACC = 8 + WQ_HUBS fp32 accumulators per lane and adjoint; per sequence they go to the workspace.
// k_pgw_sum (one wave per model and row) finds each present edge's two slots, adds both over the sequences in fp64 in
// a fixed order, rounds once and writes ALL of dA, with exact zeros wherever A[i][j] == 0.  Pad slots are summed and
// dropped.  A refused model (WqSp::sparse == 0) is left alone by the sweeps and the sums; k_gw_refuse writes NaN into
// its dA, dpi and dE rows and the call's counter.  Every offset into E, grad_out, dE and the workspace arrays is
// 64-bit.  No atomics.
//
// hmm_class_posterior_grad_walk is the same call for a loss on CLASS posteriors (sums of gamma over the states of a
// class): sweeps 3 and 4 are templated on where G comes from (PgwStateG: the (k,b,L,q) tensor, today's code;
// PgwClassG: a (k,b,L,C) tensor and the lane's class), log mode divides the upstream gradient by the class posteriors
// first (k_pgw_class_quot) and then runs in prob mode; everything else is shared.

#define PGW_PF 4                 // rows in flight per stream (k_pgw_alpha reads five streams; see DESIGN §12e)

struct PgwSums { f4 a, b; };

// the workgroup's totals of the two published quadruples, waves in order
__device__ __forceinline__ PgwSums pgw_collect(const f4 (*pa)[WQ_MAX / 64], const f4 (*pb)[WQ_MAX / 64], int s, int nw) {
    PgwSums r = {pa[s][0], pb[s][0]};
    for (int x = 1; x < nw; ++x) { r.a += pa[s][x]; r.b += pb[s][x]; }
    return r;
}

// backward value sweep: grid k*b, block NP.  RB_t = Rb_t, sign bit: the backward clamp was active.
__global__ __launch_bounds__(WQ_MAX, 4) void k_pgw_rb(const float *__restrict__ E, int b, int L, int q, float eps,
                                                   float *__restrict__ RB, const WqSp *__restrict__ sp) {
    __shared__ __attribute__((aligned(16))) float xs[2][WQ_MAX];
    __shared__ f4 part[2][WQ_MAX / 64];                       // [buffer][wave]: Sb, hub 0, hub 1
    const long long row = blockIdx.x;
    const int m = (int)(row / b);
    const WqSp &M = sp[m];
    if (!M.sparse) return;                                    // refused (block-uniform, before any barrier)
    const int i = threadIdx.x, lane = i & 63, w = i >> 6, nw = blockDim.x >> 6;
    const bool act = i < q;
    const int ic = act ? i : q - 1;
    const GwCoef c = gw_coef(M, i, true);
    const float *Er = E + (size_t)row * L * q;
    float *o = RB + (size_t)row * L * q;
    auto step = [&](const int t, const float eraw) {
        float rb = 1.f;
        bool live = true;
        if (t < L - 1) {
            f4 a = part[(t + 1) & 1][0];
            for (int x = 1; x < nw; ++x) a += part[(t + 1) & 1][x];        // waves in order
            const float *xv = xs[(t + 1) & 1];
            float r = fmaf(c.w0.w, xv[c.s0.w], fmaf(c.w0.z, xv[c.s0.z], fmaf(c.w0.y, xv[c.s0.y], c.w0.x * xv[c.s0.x])));
            r += fmaf(c.w1.w, xv[c.s1.w], fmaf(c.w1.z, xv[c.s1.z], fmaf(c.w1.y, xv[c.s1.y], c.w1.x * xv[c.s1.x])));
            r = i == c.hub0 ? a.y : (i == c.hub1 ? a.z : r);
            const float raw = r / a.x;
            live = raw > eps;
            rb = fmaxf(raw, eps);
        }
        if (act) o[(size_t)t * q + i] = live ? rb : -rb;
        const float s = act ? fmaxf(eraw, eps) * rb : 0.f;
        xs[t & 1][i] = s;
        f4 ps = {mq_wave_sum(s), 0.f, 0.f, 0.f};
        if (c.nhub > 0) ps.y = mq_wave_sum(s * c.hw0);
        if (c.nhub > 1) ps.z = mq_wave_sum(s * c.hw1);
        if (lane == 0) part[t & 1][w] = ps;
        __syncthreads();
    };
    auto erow = [&](int t) { return Er[(size_t)(t > 0 ? t : 0) * q + ic]; };
    float en[WQ_PF];
#pragma unroll
    for (int u = 0; u < WQ_PF; ++u) en[u] = erow(L - 1 - u);
    for (int tb = L - 1; tb >= 0; tb -= WQ_PF) {
#pragma unroll
        for (int u = 0; u < WQ_PF; ++u) {
            const float eraw = en[u];
            en[u] = erow(tb - u - WQ_PF);
            if (tb - u >= 0) step(tb - u, eraw);              // block-uniform
        }
    }
}

// Where the two adjoints read the upstream gradient G of (sequence, position, this lane's state).  PgwStateG: a
// (k,b,L,q) tensor, the element beside E's (hmm_posterior_grad_walk).  PgwClassG: a (k,b,L,ncls) tensor of per-class
// gradients (hmm_class_posterior_grad_walk): the class table travels by value as DecodeWide's masks, every lane finds
// its class once, and a wave's 64 lanes then touch at most ncls dwords of one or two cache lines per position.
struct PgwStateG {
    static constexpr bool cls = false;
};
struct alignas(8) PgwClassG {
    static constexpr bool cls = true;
    unsigned long long mask[QP][WQ_MAX / 64];   // bit s of mask[c]: state s belongs to class c
    int ncls;                                   // 1 .. QP
};

// lane x's class (0 for a lane beyond q: it has no bit, reads a valid element and keeps G = 0)
__device__ __forceinline__ int pgw_class_of(const PgwClassG &gs, int x) {
    const int w = x >> 6, lane = x & 63;
    int c = 0;
#pragma unroll
    for (int k = 1; k < QP; ++k)                              // (constant indices: the masks stay arguments)
#pragma unroll
        for (int u = 0; u < WQ_MAX / 64; ++u)
            if (u == w && ((gs.mask[k][u] >> lane) & 1ull)) c = k;
    return c;
}

// adjoint of the backward recursion, ascending in time: grid k*b, block NP.  Step p handles position p: it turns
// Rbar_{p-1} into w_{p-1}, gathers bhbar = A^T w_{p-1}, adds w_{p-1} (x) bh_p to the owned edges, writes dEb_p into dE
// and forms Rbar_p.  acc: (k*b, GW_ACC, NP).
template <class GS>
__device__ __forceinline__ void pgw_beta_body(const float *__restrict__ E, const float *__restrict__ AH,
                                              const float *__restrict__ RB, const float *__restrict__ G, int b, int L,
                                              int q, float eps, int mode, float *__restrict__ dE,
                                              float *__restrict__ acc, const WqSp *__restrict__ sp, const GS &gs) {
    __shared__ __attribute__((aligned(16))) float wv[WQ_MAX];
    __shared__ f4 pa[2][WQ_MAX / 64];                         // [buffer][wave]: sum U, U Rb, G U Rb, G
    __shared__ f4 pb[2][WQ_MAX / 64];                         //                 sum sb, hub 0, hub 1 (of hin w)
    __shared__ float pd[WQ_MAX / 64];                         // [wave]: sum bhbar sb
    __shared__ float hsb[WQ_HUBS];                            // sb_p[hub]
    const long long row = blockIdx.x;
    const int m = (int)(row / b);
    const WqSp &M = sp[m];
    if (!M.sparse) return;                                    // refused (block-uniform, before any barrier)
    const int x = threadIdx.x, lane = x & 63, w = x >> 6, nw = blockDim.x >> 6, NP = blockDim.x;
    const bool act = x < q;
    const int xc = act ? x : q - 1;
    const GwCoef c = gw_coef(M, x, false);
    if (x < WQ_HUBS) hsb[x] = 0.f;                            // (without hubs nobody writes them)
    const size_t base = (size_t)row * L * q;
    f4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};   // the list's edges fsrc[x][e] -> x
    float ah0 = 0.f, ah1 = 0.f;                                // the edges x -> hub
    float Rbar = 0.f, rbs = 0.f;                               // position p - 1
    auto step = [&](const int p, const float eraw, const float us, const float rb1s, const float Graw) {
        const float e1 = fmaxf(eraw, eps), rb1 = __builtin_fabsf(rb1s), G1 = act ? Graw : 0.f;
        const float u1 = act ? __builtin_fabsf(us) : 0.f;
        const float wx = (act && p > 0 && __builtin_bit_cast(int, rbs) >= 0) ? Rbar : 0.f;   // the clamp of Rb_{p-1} passes nothing
        const float sb = act ? e1 * rb1 : 0.f, ug = u1 * rb1;
        wv[x] = wx;
        if (x == c.hub0) hsb[0] = sb;
        if (x == c.hub1) hsb[1] = sb;
        f4 qa = {mq_wave_sum(u1), mq_wave_sum(ug), mq_wave_sum(G1 * ug), mq_wave_sum(G1)};
        f4 qb = {mq_wave_sum(sb), 0.f, 0.f, 0.f};
        if (c.nhub > 0) qb.y = mq_wave_sum(wx * c.hw0);
        if (c.nhub > 1) qb.z = mq_wave_sum(wx * c.hw1);
        if (lane == 0) { pa[p & 1][w] = qa; pb[p & 1][w] = qb; }
        __syncthreads();
        const PgwSums s = pgw_collect(pa, pb, p & 1, nw);
        const float iS = 1.0f / s.a.x, al1 = u1 * iS;
        float vbar = 0.f;
        if (p > 0) {                                          // block-uniform
            const float iSb = 1.0f / s.b.x, bh = sb * iSb;
            const f4 g0 = {wv[c.s0.x], wv[c.s0.y], wv[c.s0.z], wv[c.s0.w]};
            const f4 g1 = {wv[c.s1.x], wv[c.s1.y], wv[c.s1.z], wv[c.s1.w]};
            float r = fmaf(c.w0.w, g0.w, fmaf(c.w0.z, g0.z, fmaf(c.w0.y, g0.y, c.w0.x * g0.x)));
            r += fmaf(c.w1.w, g1.w, fmaf(c.w1.z, g1.z, fmaf(c.w1.y, g1.y, c.w1.x * g1.x)));
            const float bhbar = x == c.hub0 ? s.b.y : (x == c.hub1 ? s.b.z : r);
            a0.x = fmaf(g0.x, bh, a0.x); a0.y = fmaf(g0.y, bh, a0.y); a0.z = fmaf(g0.z, bh, a0.z); a0.w = fmaf(g0.w, bh, a0.w);
            a1.x = fmaf(g1.x, bh, a1.x); a1.y = fmaf(g1.y, bh, a1.y); a1.z = fmaf(g1.z, bh, a1.z); a1.w = fmaf(g1.w, bh, a1.w);
            ah0 = fmaf(wx, hsb[0] * iSb, ah0);
            ah1 = fmaf(wx, hsb[1] * iSb, ah1);
            const float d = mq_wave_sum(act ? bhbar * sb : 0.f);
            if (lane == 0) pd[w] = d;
            __syncthreads();
            float dot = pd[0];
            for (int y = 1; y < nw; ++y) dot += pd[y];        // waves in order
            vbar = act ? (bhbar - dot * iSb) * iSb : 0.f;
        }
        if (act) dE[base + (size_t)p * q + x] = vbar * rb1;   // (bh_0 feeds nothing)
        float ga, gr;
        pgl_local(G1, al1, rb1, act, mode, s.a.y * iS, s.a.z * iS, s.a.w, &ga, &gr);
        Rbar = ga + vbar * e1;
        rbs = rb1s;
    };
    auto at = [&](int t) { return base + (size_t)(t < L ? t : L - 1) * q + xc; };
    const float *gp = G;                                       // PgwClassG: the sequence's row 0 (block-uniform) ...
    unsigned cls = 0;                                          // ... and this lane's class: the one per-lane offset
    int C = 0;
    if constexpr (GS::cls) { C = gs.ncls; gp = G + (size_t)row * L * C; cls = pgw_class_of(gs, x) & (QP - 1); }
    auto gat = [&](int t, size_t o) -> float {                 // G of position min(t, L - 1); o = at(t)
        if constexpr (GS::cls) return (gp + (size_t)(t < L ? t : L - 1) * C)[cls];
        else return G[o];
    };
    float en[PGW_PF], un[PGW_PF], rn[PGW_PF], gn[PGW_PF];
#pragma unroll
    for (int u = 0; u < PGW_PF; ++u) { const size_t o = at(u); en[u] = E[o]; un[u] = AH[o]; rn[u] = RB[o]; gn[u] = gat(u, o); }
    for (int tb = 0; tb < L; tb += PGW_PF) {
#pragma unroll
        for (int u = 0; u < PGW_PF; ++u) {
            const float e = en[u], us = un[u], r = rn[u], g = gn[u];
            const size_t o = at(tb + u + PGW_PF);
            en[u] = E[o]; un[u] = AH[o]; rn[u] = RB[o]; gn[u] = gat(tb + u + PGW_PF, o);
            if (tb + u < L) step(tb + u, e, us, r, g);        // block-uniform
        }
    }
    float *ar = acc + (size_t)row * GW_ACC * NP + x;
    ar[0 * NP] = a0.x; ar[1 * NP] = a0.y; ar[2 * NP] = a0.z; ar[3 * NP] = a0.w;
    ar[4 * NP] = a1.x; ar[5 * NP] = a1.y; ar[6 * NP] = a1.z; ar[7 * NP] = a1.w;
    ar[8 * NP] = ah0;  ar[9 * NP] = ah1;
}

__global__ __launch_bounds__(WQ_MAX, 4) void k_pgw_beta(const float *__restrict__ E, const float *__restrict__ AH,
                                                     const float *__restrict__ RB, const float *__restrict__ G, int b,
                                                     int L, int q, float eps, int mode, float *__restrict__ dE,
                                                     float *__restrict__ acc, const WqSp *__restrict__ sp) {
    pgw_beta_body(E, AH, RB, G, b, L, q, eps, mode, dE, acc, sp, PgwStateG());
}

// the same with per-class gradients: Gs (k,b,L,gs.ncls).  (Five workgroups per CU asked for: the state form reaches
// them at 92 VGPRs on its own, this one needs telling to stay within 96.)
__global__ __launch_bounds__(WQ_MAX, 5) void k_pgw_beta_class(const float *__restrict__ E, const float *__restrict__ AH,
                                                           const float *__restrict__ RB, const float *__restrict__ Gs,
                                                           int b, int L, int q, float eps, int mode,
                                                           float *__restrict__ dE, float *__restrict__ acc,
                                                           const WqSp *__restrict__ sp, const PgwClassG gs) {
    pgw_beta_body(E, AH, RB, Gs, b, L, q, eps, mode, dE, acc, sp, gs);
}

// adjoint of the forward recursion, descending in time: grid k*b, block NP.  Step t normalises U_t, adds
// alpha_hat_t (x) Rfbar_{t+1} (gathered by the step before) to the owned edges, finishes dE_t in place (dE holds the
// share of k_pgw_beta) and gathers abar_{t-1} = A Rfbar_t; at t = 0 the sequence's dpi.  acc: (k*b, GW_ACC, NP).
template <class GS>
__device__ __forceinline__ void pgw_alpha_body(const float *__restrict__ pi, const float *__restrict__ E,
                                               const float *__restrict__ AH, const float *__restrict__ RB,
                                               const float *__restrict__ G, int b, int L, int q, float eps, int mode,
                                               float *__restrict__ dE, float *__restrict__ acc,
                                               float *__restrict__ dpi_part, const WqSp *__restrict__ sp,
                                               const GS &gs) {
    __shared__ __attribute__((aligned(16))) float rv[WQ_MAX];
    __shared__ f4 pa[1][WQ_MAX / 64];                         // [wave]: sum U, U Rb, G U Rb, G
    __shared__ f4 pb[1][WQ_MAX / 64];                         //         sum G (U > 0), abar U
    __shared__ float ph[WQ_HUBS][WQ_MAX / 64];                // [hub][wave]: sum hout Rfbar
    __shared__ float hal[WQ_HUBS];                            // |U_t[hub]|
    const long long row = blockIdx.x;
    const int m = (int)(row / b);
    const WqSp &M = sp[m];
    if (!M.sparse) return;                                    // refused (block-uniform, before any barrier)
    const int x = threadIdx.x, lane = x & 63, w = x >> 6, nw = blockDim.x >> 6, NP = blockDim.x;
    const bool act = x < q;
    const int xc = act ? x : q - 1;
    const GwCoef c = gw_coef(M, x, true);
    if (x < WQ_HUBS) hal[x] = 0.f;                            // (without hubs nobody writes them)
    const size_t base = (size_t)row * L * q;
    f4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};   // the list's edges x -> bsrc[x][e]
    f4 p0 = {0.f, 0.f, 0.f, 0.f}, p1 = {0.f, 0.f, 0.f, 0.f};   // what the step before gathered: Rfbar_{t+1} at bsrc
    float ah0 = 0.f, ah1 = 0.f;                                // the edges hub -> x
    float abar = 0.f, rfn = 0.f;                               // d loss / d alpha_hat_t from the future; Rfbar_{t+1}[x]
    auto step = [&](const int t, const float eraw, const float us, const float rbs, const float Graw, const float deb) {
        const float e = fmaxf(eraw, eps), rb = __builtin_fabsf(rbs), Gt = act ? Graw : 0.f;
        const float u = act ? __builtin_fabsf(us) : 0.f, ug = u * rb;
        if (x == c.hub0) hal[0] = u;
        if (x == c.hub1) hal[1] = u;
        f4 qa = {mq_wave_sum(u), mq_wave_sum(ug), mq_wave_sum(Gt * ug), mq_wave_sum(Gt)};
        f4 qb = {mq_wave_sum(u > 0.f ? Gt : 0.f), mq_wave_sum(abar * u), 0.f, 0.f};
        if (lane == 0) { pa[0][w] = qa; pb[0][w] = qb; }
        __syncthreads();
        const PgwSums s = pgw_collect(pa, pb, 0, nw);
        const float S = s.a.x, iS = 1.0f / S, al = u * iS, Sg = s.a.y * iS, SGg = s.a.z * iS;
        // alpha_hat_t (x) Rfbar_{t+1}: zeros at t = L - 1
        a0.x = fmaf(al, p0.x, a0.x); a0.y = fmaf(al, p0.y, a0.y); a0.z = fmaf(al, p0.z, a0.z); a0.w = fmaf(al, p0.w, a0.w);
        a1.x = fmaf(al, p1.x, a1.x); a1.y = fmaf(al, p1.y, a1.y); a1.z = fmaf(al, p1.z, a1.z); a1.w = fmaf(al, p1.w, a1.w);
        ah0 = fmaf(hal[0] * iS, rfn, ah0);
        ah1 = fmaf(hal[1] * iS, rfn, ah1);
        float ga, gr;
        pgl_local(Gt, al, rb, act, mode, Sg, SGg, s.a.w, &ga, &gr);
        const float dot = s.b.y * iS + pgl_gr_dot_al(mode, Sg, SGg, s.a.w, s.b.x);
        const float ubar = act ? (abar + gr - dot) / S : 0.f;
        if (act) dE[base + (size_t)t * q + x] = eraw > eps ? deb + ubar * (u / e) : 0.f;   // u_t / E'_t = max(R^f_t, eps)
        const float Rfbar = (act && __builtin_bit_cast(int, us) >= 0) ? ubar * e : 0.f;     // the clamp of R^f_t passes nothing
        if (t > 0) {                                          // block-uniform
            rv[x] = Rfbar;
            float h0 = 0.f, h1 = 0.f;
            if (c.nhub > 0) h0 = mq_wave_sum(Rfbar * c.hw0);
            if (c.nhub > 1) h1 = mq_wave_sum(Rfbar * c.hw1);
            if (lane == 0) { ph[0][w] = h0; ph[1][w] = h1; }
            __syncthreads();
            h0 = ph[0][0]; h1 = ph[1][0];
            for (int y = 1; y < nw; ++y) { h0 += ph[0][y]; h1 += ph[1][y]; }   // waves in order
            p0 = (f4){rv[c.s0.x], rv[c.s0.y], rv[c.s0.z], rv[c.s0.w]};
            p1 = (f4){rv[c.s1.x], rv[c.s1.y], rv[c.s1.z], rv[c.s1.w]};
            float r = fmaf(c.w0.w, p0.w, fmaf(c.w0.z, p0.z, fmaf(c.w0.y, p0.y, c.w0.x * p0.x)));
            r += fmaf(c.w1.w, p1.w, fmaf(c.w1.z, p1.z, fmaf(c.w1.y, p1.y, c.w1.x * p1.x)));
            r = x == c.hub0 ? h0 : (x == c.hub1 ? h1 : r);
            abar = act ? r : 0.f;                             // (A Rfbar_t)[x]
            rfn = Rfbar;
        } else if (act) {
            dpi_part[(size_t)row * q + x] = pi[(size_t)m * q + x] > eps ? Rfbar : 0.f;
        }
    };
    // the rings run towards position 0; positions before the start re-read row 0.  dE_t is read here before the step of
    // position t writes it (each lane reads and writes its own element only).
    auto at = [&](int t) { return base + (size_t)(t > 0 ? t : 0) * q + xc; };
    const float *gp = G;                                       // PgwClassG: the sequence's row 0 (block-uniform) ...
    unsigned cls = 0;                                          // ... and this lane's class: the one per-lane offset
    int C = 0;
    if constexpr (GS::cls) { C = gs.ncls; gp = G + (size_t)row * L * C; cls = pgw_class_of(gs, x) & (QP - 1); }
    auto gat = [&](int t, size_t o) -> float {                 // G of position max(t, 0); o = at(t)
        if constexpr (GS::cls) return (gp + (size_t)(t > 0 ? t : 0) * C)[cls];
        else return G[o];
    };
    float en[PGW_PF], un[PGW_PF], rn[PGW_PF], gn[PGW_PF], dn[PGW_PF];
#pragma unroll
    for (int u = 0; u < PGW_PF; ++u) {
        const size_t o = at(L - 1 - u);
        en[u] = E[o]; un[u] = AH[o]; rn[u] = RB[o]; gn[u] = gat(L - 1 - u, o); dn[u] = dE[o];
    }
    __syncthreads();                                          // hal zeroed
    for (int tb = L - 1; tb >= 0; tb -= PGW_PF) {
#pragma unroll
        for (int u = 0; u < PGW_PF; ++u) {
            const float e = en[u], us = un[u], r = rn[u], g = gn[u], d = dn[u];
            const size_t o = at(tb - u - PGW_PF);
            en[u] = E[o]; un[u] = AH[o]; rn[u] = RB[o]; gn[u] = gat(tb - u - PGW_PF, o); dn[u] = dE[o];
            if (tb - u >= 0) step(tb - u, e, us, r, g, d);    // block-uniform
        }
    }
    float *ar = acc + (size_t)row * GW_ACC * NP + x;
    ar[0 * NP] = a0.x; ar[1 * NP] = a0.y; ar[2 * NP] = a0.z; ar[3 * NP] = a0.w;
    ar[4 * NP] = a1.x; ar[5 * NP] = a1.y; ar[6 * NP] = a1.z; ar[7 * NP] = a1.w;
    ar[8 * NP] = ah0;  ar[9 * NP] = ah1;
}

__global__ __launch_bounds__(WQ_MAX, 4) void k_pgw_alpha(const float *__restrict__ pi, const float *__restrict__ E,
                                                      const float *__restrict__ AH, const float *__restrict__ RB,
                                                      const float *__restrict__ G, int b, int L, int q, float eps,
                                                      int mode, float *__restrict__ dE, float *__restrict__ acc,
                                                      float *__restrict__ dpi_part, const WqSp *__restrict__ sp) {
    pgw_alpha_body(pi, E, AH, RB, G, b, L, q, eps, mode, dE, acc, dpi_part, sp, PgwStateG());
}

// the same with per-class gradients: Gs (k,b,L,gs.ncls)
__global__ __launch_bounds__(WQ_MAX, 4) void k_pgw_alpha_class(const float *__restrict__ pi, const float *__restrict__ E,
                                                            const float *__restrict__ AH, const float *__restrict__ RB,
                                                            const float *__restrict__ Gs, int b, int L, int q,
                                                            float eps, int mode, float *__restrict__ dE,
                                                            float *__restrict__ acc, float *__restrict__ dpi_part,
                                                            const WqSp *__restrict__ sp, const PgwClassG gs) {
    pgw_alpha_body(pi, E, AH, RB, Gs, b, L, q, eps, mode, dE, acc, dpi_part, sp, gs);
}

// log mode's upstream gradient in prob-mode terms: Gp = grad_out / class_prob (the IEEE fp32 quotient), 0 where the
// class posterior is 0 (an empty or exactly-zero class passes nothing).  n = k b L ncls elements, grid-stride.
__global__ __launch_bounds__(256) void k_pgw_class_quot(const float *__restrict__ g, const float *__restrict__ P,
                                                        float *__restrict__ Gp, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const float p = P[i];
        Gp[i] = p > 0.f ? g[i] / p : 0.f;
    }
}

// dA (k,q,q) from the sequences' accumulators of both adjoints: one wave per (model, row i).  Every entry of the row is
// written: 0 where A[i][j] == 0, else the two owners' slots summed over the model's b sequences in fp64 (lane s takes
// sequences s, s + 64, ..., then a fixed butterfly) and rounded once.
//   accb (sweep 3)   i -> j, j not a hub: slot e of lane j with fsrc[j][e] == i;  i -> hub h: slot 8 + h of lane i
//   acca (sweep 4)   i -> j, i not a hub: slot e of lane i with bsrc[i][e] == j;  hub h -> j: slot 8 + h of lane j
__global__ __launch_bounds__(64) void k_pgw_sum(const float *__restrict__ accb, const float *__restrict__ acca,
                                                float *__restrict__ dA, int b, int q, int NP,
                                                const WqSp *__restrict__ sp) {
    const int m = blockIdx.y, i = blockIdx.x, tid = threadIdx.x;
    const WqSp &M = sp[m];
    if (!M.sparse) return;                                    // refused: k_gw_refuse writes this model's dA
    const int h = i == M.hub[0] ? 0 : (i == M.hub[1] ? 1 : -1);
    float *row = dA + ((size_t)m * q + i) * q;
    const size_t om = (size_t)m * b * GW_ACC * NP;
    auto edge = [&](int j, int sa, int la) {                  // sweep 4's slot and lane given; sweep 3's found here
        int sb = 0, lb = 0;
        if (j == M.hub[0] || j == M.hub[1]) {
            sb = WQ_SP_MAX + (j == M.hub[0] ? 0 : 1); lb = i;
        } else {
            lb = j;
            for (int e = 0; e < WQ_SP_MAX; ++e)
                if (M.fsrc[j][e] == i && M.fw[j][e] != 0.f) sb = e;
        }
        double s = 0.0;
        for (int r = tid; r < b; r += 64)
            s += (double)acca[om + ((size_t)r * GW_ACC + sa) * NP + la] + (double)accb[om + ((size_t)r * GW_ACC + sb) * NP + lb];
        s = pg_wave_sum_d(s);
        if (tid == 0) row[j] = (float)s;
    };
    for (int j = tid; j < q; j += 64) row[j] = 0.f;
    __syncthreads();                                          // (one wave: orders the zeros before the entries)
    if (h >= 0) {                                             // a hub's row: lane j owns h -> j in sweep 4
        for (int j = 0; j < q; ++j)
            if (M.hout[h][j] != 0.f) edge(j, WQ_SP_MAX + h, j);               // wave-uniform
        return;
    }
    for (int e = 0; e < WQ_SP_MAX; ++e)
        if (M.bw[i][e] != 0.f) edge(M.bsrc[i][e], e, i);      // else a pad; wave-uniform
}

// ---- host side
struct PgwPlan { int NP; size_t o_ll, o_sp, o_count, o_dpi, o_accb, o_acca, o_ah, o_rb, total; };
static int make_pgwplan(int k, int b, int L, int q, PgwPlan *p) {
    if (k < 1 || b < 1 || L < 1 || q < 1) return HMM_ERR_BAD_SHAPE;
    if (q < WQ_MIN || q > WQ_MAX) return HMM_ERR_Q_UNSUPPORTED;
    p->NP = (q + 63) / 64 * 64;
    const size_t nr = (size_t)k * b, seq = nr * L * q * sizeof(float), part = nr * GW_ACC * p->NP * sizeof(float);
    size_t off = 0;
    p->o_ll = off;    off = align_up(off + nr * sizeof(double));
    p->o_sp = off;    off = align_up(off + (size_t)k * sizeof(WqSp));
    p->o_count = off; off = align_up(off + sizeof(int));
    p->o_dpi = off;   off = align_up(off + nr * q * sizeof(float));               // dpi per sequence
    p->o_accb = off;  off = align_up(off + part);                                 // sweep 3's edge accumulators
    p->o_acca = off;  off = align_up(off + part);                                 // sweep 4's
    p->o_ah = off;    off = align_up(off + seq);                                  // signed U_t
    p->o_rb = off;    off = align_up(off + seq);                                  // signed Rb_t
    p->total = off;
    return HMM_OK;
}

extern "C" {

int hmm_posterior_grad_walk_min_states(void) { return WQ_MIN; }
int hmm_posterior_grad_walk_max_states(void) { return WQ_MAX; }

size_t hmm_posterior_grad_walk_workspace_bytes(int k, int b, int L, int q) {
    PgwPlan p;
    return make_pgwplan(k, b, L, q, &p) ? 0 : p.total;
}

// 1 where this call measured at least 1.25x faster than hmm_posterior_grad_large at its default route (DESIGN §12e;
// tools/experiments/posterior_grad_walk_time.py, profiles/posterior_grad_walk.json); 0 where nothing was measured.
// Measured on one MI355X at L = 10 000, one model, 1 / 32 / 1024 sequences, log mode, a label-style upstream gradient:
// 2.8 .. 3.6x at 71 states and 3.4 .. 6.4x at 127 (against the dense walk), 14 .. 21x at 253 (against the per-position
// GEMMs) — every cell pays, so the rule is the measured range itself, as for hmm_loglik_grad_walk_pays: up to
// PGW_PAYS_SEQS sequences in the call.  More sequences were not measured.  L does not enter: both evaluations cost
// per position.  Only models inside the sparse rule were measured (others are refused).
#define PGW_PAYS_SEQS 1024
int hmm_posterior_grad_walk_pays(int k, int b, int L, int q) {
    PgwPlan p;
    if (make_pgwplan(k, b, L, q, &p)) return 0;
    return (long long)k * b <= PGW_PAYS_SEQS ? 1 : 0;
}

long long hmm_posterior_grad_walk_refused(int k, int b, int L, int q, const void *workspace, size_t workspace_bytes) {
    PgwPlan p;
    int rc = make_pgwplan(k, b, L, q, &p);
    if (rc) return rc;
    if (!workspace) return HMM_ERR_NULL_POINTER;
    if (workspace_bytes < p.total) return HMM_ERR_WORKSPACE;
    int v = 0;
    if (hipMemcpy(&v, ws_at<int>(workspace, p.o_count), sizeof(int), hipMemcpyDeviceToHost) != hipSuccess)
        return HMM_ERR_LAUNCH;
    return v;
}

int hmm_posterior_grad_walk(const float *A, const float *pi, const float *E, int k, int b, int L, int q, float eps,
                            int mode, const float *grad_out, float *dA, float *dpi, float *dE, void *workspace,
                            size_t workspace_bytes, void *stream) {
    PgwPlan p;
    int rc = make_pgwplan(k, b, L, q, &p);
    if (rc) return rc;
    if (mode != HMM_POST_PROB && mode != HMM_POST_LOG) return HMM_ERR_BAD_ARGUMENT;
    if (!A || !pi || !E || !grad_out || !dA || !dpi || !dE || !workspace) return HMM_ERR_NULL_POINTER;
    if ((rc = check_eps(eps))) return rc;
    if ((rc = check_ws(p.total, workspace, workspace_bytes))) return rc;
    hipStream_t st = (hipStream_t)stream;
    WqSp *sp = ws_at<WqSp>(workspace, p.o_sp);
    const WqSp *csp = sp;
    double *ll = ws_at<double>(workspace, p.o_ll);
    float *AH = ws_at<float>(workspace, p.o_ah), *RB = ws_at<float>(workspace, p.o_rb);
    float *accb = ws_at<float>(workspace, p.o_accb), *acca = ws_at<float>(workspace, p.o_acca);
    float *dpp = ws_at<float>(workspace, p.o_dpi);
    const float *cAH = AH, *cRB = RB;
    const dim3 grid((unsigned)((size_t)k * b)), blk((unsigned)p.NP);
    launch(k_wq_prep, dim3(k), dim3(WQ_MAX), 0, st, A, sp, q, 0);
    launch(k_gw_fwd<true>, grid, blk, 0, st, pi, E, b, L, q, eps, AH, ll, csp);
    launch(k_pgw_rb, grid, blk, 0, st, E, b, L, q, eps, RB, csp);
    launch(k_pgw_beta, grid, blk, 0, st, E, cAH, cRB, grad_out, b, L, q, eps, mode, dE, accb, csp);
    launch(k_pgw_alpha, grid, blk, 0, st, pi, E, cAH, cRB, grad_out, b, L, q, eps, mode, dE, acca, dpp, csp);
    launch(k_pgw_sum, dim3(q, k), dim3(64), 0, st, (const float *)accb, (const float *)acca, dA, b, q, p.NP, csp);
    launch(k_pg_sum_rows, dim3(q, k), dim3(64), 0, st, (const float *)dpp, dpi, b, q);
    launch(k_gw_refuse, dim3(GW_REFUSE_BLOCKS, k), dim3(256), 0, st, csp, k, b, L, q, dA, dpi, dE, ll,
           ws_at<int>(workspace, p.o_count));
    return check_launch();
}

// hmm_posterior_grad_walk's layout first (hmm_posterior_grad_walk_refused reads the counter of a finished call of
// either kind), then log mode's quotient tensor (k,b,L,num_classes)
size_t hmm_class_posterior_grad_walk_workspace_bytes(int k, int b, int L, int q, int num_classes) {
    PgwPlan p;
    if (make_pgwplan(k, b, L, q, &p) || num_classes < 1 || num_classes > QP) return 0;
    return align_up(p.total) + align_up((size_t)k * b * L * num_classes * sizeof(float));
}

int hmm_class_posterior_grad_walk(const float *A, const float *pi, const float *E, int k, int b, int L, int q, float eps,
                                  int mode, const int *state_class, int num_classes, const float *class_prob,
                                  const float *grad_out, float *dA, float *dpi, float *dE, void *workspace,
                                  size_t workspace_bytes, void *stream) {
    PgwPlan p;
    int rc = make_pgwplan(k, b, L, q, &p);
    if (rc) return rc;
    if (mode != HMM_POST_PROB && mode != HMM_POST_LOG) return HMM_ERR_BAD_ARGUMENT;
    if (!A || !pi || !E || !state_class || !grad_out || !dA || !dpi || !dE || !workspace ||
        (mode == HMM_POST_LOG && !class_prob))
        return HMM_ERR_NULL_POINTER;
    if (num_classes < 1 || num_classes > QP || check_eps(eps)) return HMM_ERR_BAD_ARGUMENT;
    PgwClassG gs{};
    gs.ncls = num_classes;
    for (int s = 0; s < q; ++s) {                              // the table is read here, once, and travels by value
        if (state_class[s] < 0 || state_class[s] >= num_classes) return HMM_ERR_BAD_ARGUMENT;
        gs.mask[state_class[s]][s >> 6] |= 1ull << (s & 63);
    }
    const size_t o_gp = align_up(p.total), ng = (size_t)k * b * L * num_classes;
    if ((rc = check_ws(o_gp + align_up(ng * sizeof(float)), workspace, workspace_bytes))) return rc;
    hipStream_t st = (hipStream_t)stream;
    WqSp *sp = ws_at<WqSp>(workspace, p.o_sp);
    const WqSp *csp = sp;
    double *ll = ws_at<double>(workspace, p.o_ll);
    float *AH = ws_at<float>(workspace, p.o_ah), *RB = ws_at<float>(workspace, p.o_rb);
    float *accb = ws_at<float>(workspace, p.o_accb), *acca = ws_at<float>(workspace, p.o_acca);
    float *dpp = ws_at<float>(workspace, p.o_dpi);
    const float *cAH = AH, *cRB = RB, *Gs = grad_out;
    if (mode == HMM_POST_LOG) {                                // d/d gamma_j of sum Gc log P = Gc / P at j's class
        float *Gp = ws_at<float>(workspace, o_gp);
        const size_t nb = (ng + 255) / 256;
        launch(k_pgw_class_quot, dim3((unsigned)(nb < 65536 ? nb : 65536)), dim3(256), 0, st, grad_out, class_prob, Gp, ng);
        Gs = Gp;
    }
    const dim3 grid((unsigned)((size_t)k * b)), blk((unsigned)p.NP);
    launch(k_wq_prep, dim3(k), dim3(WQ_MAX), 0, st, A, sp, q, 0);
    launch(k_gw_fwd<true>, grid, blk, 0, st, pi, E, b, L, q, eps, AH, ll, csp);
    launch(k_pgw_rb, grid, blk, 0, st, E, b, L, q, eps, RB, csp);
    launch(k_pgw_beta_class, grid, blk, 0, st, E, cAH, cRB, Gs, b, L, q, eps, (int)HMM_POST_PROB, dE, accb, csp, gs);
    launch(k_pgw_alpha_class, grid, blk, 0, st, pi, E, cAH, cRB, Gs, b, L, q, eps, (int)HMM_POST_PROB, dE, acca, dpp, csp,
           gs);
    launch(k_pgw_sum, dim3(q, k), dim3(64), 0, st, (const float *)accb, (const float *)acca, dA, b, q, p.NP, csp);
    launch(k_pg_sum_rows, dim3(q, k), dim3(64), 0, st, (const float *)dpp, dpi, b, q);
    launch(k_gw_refuse, dim3(GW_REFUSE_BLOCKS, k), dim3(256), 0, st, csp, k, b, L, q, dA, dpi, dE, ll,
           ws_at<int>(workspace, p.o_count));
    return check_launch();
}

}  // extern "C"
