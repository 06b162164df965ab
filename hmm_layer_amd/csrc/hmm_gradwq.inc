// hmm_gradwq.inc — log-likelihoods and their gradients for 65 <= q <= 256 states by a per-sequence walk with the sparse
// step (hmm_loglik_grad_walk), included by hmm_engine.hip after hmm_wideq.inc and hmm_grad_large.inc.
//
// The derivatives and the clamp handling are those stated at the top of hmm_grad_large.inc, and so are the two
// launches: a forward sweep over all L positions that parks the signed unnormalised forward vector U_t in the caller's
// dE (sign bit: the state was not live), then a backward sweep that overwrites it position by position with dE_t and
// collects dA; k_mq_grad_pi sums dpi from position 0 and zeroes its clamped entries.  What differs is the step: the
// lists, hub columns and verdict of k_wq_prep (hmm_wideq.inc, called with force_dense = 0: HMM_OPT_FORCE_DENSE does
// not act here).  One workgroup per sequence, NP = 64 ceil(q/64) threads, lane = state.
//
//   forward   lane j gathers its <= 8 (fsrc, fw) pairs from the LDS vector (increasing source index, four products then
//             four); a hub's predicted mass is the workgroup-wide sum of x[i] hin[h][i].
//   backward  lane i gathers bh_{t+1}[bsrc[i][e]] bw[i][e] for R_t; a hub's R_t is the sum of hout[h][j] bh_{t+1}[j].
//
// Each sweep keeps its vector in LDS, double-buffered, with ONE barrier per step: the wave sums a step needs (the
// normaliser, the row sum of gamma, the hub sums) are published per wave before the barrier and added in wave order by
// every lane after it.  The backward sweep therefore finishes position t + 1 during step t, as k_gl_walk_bwd does.
// WQ_PF rows of E (backward: and of U) are kept in flight.  Every offset into E and dE is 64-bit.  No atomics.
//
// dA on the support of A.  Every non-zero edge has exactly one owner, which sums it in an fp32 register over the
// sequence:
//   edge i -> j, i not a hub   lane i, slot e of its successor list: coef_t[i] bh_{t+1}[bsrc[i][e]], the very values
//                              the mat-vec of the step before gathered (kept in registers for one step);
//   edge h -> j out of hub h   lane j (hub targets included): coef_t[h] bh_{t+1}[j]; lane h publishes |U_t[h]| in LDS
//                              and every lane forms coef_t[h] from it and the workgroup-uniform scales.
// That is GW_ACC = 8 + WQ_HUBS accumulators per lane.  Pad slots (weight 0) are summed and dropped.  The sequences'
// accumulators go to the workspace (NP GW_ACC floats each); k_gw_sum adds them in fp64 in a fixed order, rounds once
// and writes ALL of dA: the owned entries, and an exact 0 wherever A[i][j] == 0.
//
// A model outside the sparse rule (WqSp::sparse == 0: more than WQ_HUBS states above degree 8) is refused on the
// device: the sweeps leave it alone, k_gw_refuse writes NaN into every element of its dA, dpi, dE rows and loglik, and
// the call's counter in the workspace (hmm_loglik_grad_walk_refused) says how many of the k models were refused.

#define GW_ACC (WQ_SP_MAX + WQ_HUBS)
#define GW_REFUSE_BLOCKS 64

struct GwCoef {                  // this lane's list, its entries into / out of the hubs, the hubs
    i4 s0, s1;
    f4 w0, w1;
    float hw0, hw1;
    int hub0, hub1, nhub;
};

__device__ __forceinline__ GwCoef gw_coef(const WqSp &M, int j, bool back) {
    GwCoef c;
    const int (*src)[WQ_SP_MAX] = back ? M.bsrc : M.fsrc;
    const float (*wt)[WQ_SP_MAX] = back ? M.bw : M.fw;
    c.s0 = *reinterpret_cast<const i4 *>(&src[j][0]); c.s1 = *reinterpret_cast<const i4 *>(&src[j][4]);
    c.w0 = *reinterpret_cast<const f4 *>(&wt[j][0]);  c.w1 = *reinterpret_cast<const f4 *>(&wt[j][4]);
    c.hw0 = back ? M.hout[0][j] : M.hin[0][j];
    c.hw1 = back ? M.hout[1][j] : M.hin[1][j];
    c.nhub = M.nhub; c.hub0 = M.hub[0]; c.hub1 = M.hub[1];
    return c;
}

// forward: grid k*b, block NP.  Writes the fp64 log-likelihood and, with GRAD, signed U_t into dE.
template <bool GRAD>
__global__ __launch_bounds__(WQ_MAX) void k_gw_fwd(const float *__restrict__ pi, const float *__restrict__ E, int b, int L,
                                                   int q, float eps, float *__restrict__ dE, double *__restrict__ ll,
                                                   const WqSp *__restrict__ sp) {
    __shared__ __attribute__((aligned(16))) float xs[2][WQ_MAX];
    __shared__ f4 part[2][WQ_MAX / 64];                       // [buffer][wave]: S, hub 0, hub 1
    const long long row = blockIdx.x;
    const int m = (int)(row / b);
    const WqSp &M = sp[m];
    if (!M.sparse) return;                                    // refused (block-uniform, before any barrier)
    const int j = threadIdx.x, lane = j & 63, w = j >> 6, nw = blockDim.x >> 6;
    const bool act = j < q;
    const int jc = act ? j : q - 1;
    const GwCoef c = gw_coef(M, j, false);
    const float *Er = E + (size_t)row * L * q;
    float *o = GRAD ? dE + (size_t)row * L * q : nullptr;
    double lacc = 0.0;
    auto step = [&](const int t, const float eraw) {
        float R;
        if (t == 0) {
            R = pi[(size_t)m * q + jc];
        } else {
            f4 a = part[(t - 1) & 1][0];
            for (int x = 1; x < nw; ++x) a += part[(t - 1) & 1][x];      // waves in order
            lacc += (double)logf(a.x);
            const float *xv = xs[(t - 1) & 1];
            float r = fmaf(c.w0.w, xv[c.s0.w], fmaf(c.w0.z, xv[c.s0.z], fmaf(c.w0.y, xv[c.s0.y], c.w0.x * xv[c.s0.x])));
            r += fmaf(c.w1.w, xv[c.s1.w], fmaf(c.w1.z, xv[c.s1.z], fmaf(c.w1.y, xv[c.s1.y], c.w1.x * xv[c.s1.x])));
            r = j == c.hub0 ? a.y : (j == c.hub1 ? a.z : r);
            R = r * __builtin_amdgcn_rcpf(a.x);
        }
        const float sf = act ? fmaxf(eraw, eps) * fmaxf(R, eps) : 0.f;
        if constexpr (GRAD) {
            if (act) o[(size_t)t * q + j] = R > eps ? sf : -sf;
        }
        xs[t & 1][j] = sf;
        f4 ps = {mq_wave_sum(sf), 0.f, 0.f, 0.f};
        if (c.nhub > 0) ps.y = mq_wave_sum(sf * c.hw0);
        if (c.nhub > 1) ps.z = mq_wave_sum(sf * c.hw1);
        if (lane == 0) part[t & 1][w] = ps;
        __syncthreads();
    };
    // a ring of WQ_PF emission rows in flight: a step's register is reloaded with the row WQ_PF positions ahead as soon
    // as the step has taken its value; positions past the end re-read the last row (no branch around the loads)
    auto erow = [&](int t) { return Er[(size_t)(t < L ? t : L - 1) * q + jc]; };
    float en[WQ_PF];
#pragma unroll
    for (int u = 0; u < WQ_PF; ++u) en[u] = erow(u);
    for (int tb = 0; tb < L; tb += WQ_PF) {
#pragma unroll
        for (int u = 0; u < WQ_PF; ++u) {
            const float eraw = en[u];
            en[u] = erow(tb + u + WQ_PF);
            if (tb + u < L) step(tb + u, eraw);               // block-uniform
        }
    }
    if (j == 0) {
        float S = part[(L - 1) & 1][0].x;
        for (int x = 1; x < nw; ++x) S += part[(L - 1) & 1][x].x;
        ll[row] = lacc + (double)logf(S);
    }
}

// backward: grid k*b, block NP.  Step t forms R_t from the masked bh_{t+1} in LDS and publishes the masked
// sb_t = max(E_t, eps) R_t with the per-wave sums of g_t = |U_t| R_t, of the unmasked sb_t and of the hub products; the
// same step, with the sums of position t + 1 now visible, writes dE_{t+1} and adds coef_{t+1} bh_{t+2} to the owned
// edges.  acc: (k*b, GW_ACC, NP).  (Four waves per SIMD: at most 128 VGPRs, so that four 4-wave workgroups share a CU.)
__global__ __launch_bounds__(WQ_MAX, 4) void k_gw_bwd(const float *__restrict__ E, int b, int L, int q, float eps,
                                                   const float *__restrict__ gw, float *__restrict__ dE,
                                                   float *__restrict__ acc, const WqSp *__restrict__ sp) {
    __shared__ __attribute__((aligned(16))) float sb[2][WQ_MAX];
    __shared__ f4 part[2][WQ_MAX / 64];                       // [buffer][wave]: sum g, sum sb (unmasked), hub 0, hub 1
    __shared__ float hal[2][WQ_HUBS];                         // [buffer][hub]: |U_t[hub]|
    const long long row = blockIdx.x;
    const int m = (int)(row / b);
    const WqSp &M = sp[m];
    if (!M.sparse) return;                                    // refused (block-uniform, before any barrier)
    const int i = threadIdx.x, lane = i & 63, w = i >> 6, nw = blockDim.x >> 6, NP = blockDim.x;
    const bool act = i < q;
    const int ic = act ? i : q - 1;
    const GwCoef c = gw_coef(M, i, true);
    if (i < 2 * WQ_HUBS) hal[i >> 1][i & 1] = 0.f;            // (without hubs nobody writes them)
    const float *Er = E + (size_t)row * L * q;
    float *o = dE + (size_t)row * L * q;
    const float wt = gw ? gw[row] : 1.f;
    f4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};   // the list's edges
    f4 p0 = {0.f, 0.f, 0.f, 0.f}, p1 = {0.f, 0.f, 0.f, 0.f};   // what the step before gathered: bh_{t+2} at bsrc
    float ah0 = 0.f, ah1 = 0.f;                                // the edges hub -> this lane
    float own = 0.f, ownp = 0.f;                               // this lane's masked sb_{t+1}, sb_{t+2}
    float gprev = 0.f, eprev = 0.f, alprev = 0.f, ib2 = 0.f;   // position t + 1: g, raw E, |U|; 1 / Sb_{t+2}
    auto sums = [&](int s) {
        f4 a = part[s][0];
        for (int x = 1; x < nw; ++x) a += part[s][x];          // waves in order
        return a;
    };
    // dE of position t1 from its published sums; returns w / Sg.  Position 0 keeps w gamma_0 / eps in its clamped
    // entries for k_mq_grad_pi, which zeroes them.
    auto finish = [&](int t1, float Sg) {
        const float sc = wt / Sg;
        if (act) o[(size_t)t1 * q + i] = (eprev > eps || t1 == 0) ? gprev * sc / fmaxf(eprev, eps) : 0.f;
        return sc;
    };
    // coef_{t1} bh_{t1+1} into the owned edges: cm = (w / Sg_{t1}) / Sb_{t1+1}, workgroup-uniform
    auto outer = [&](int t1, float cm) {
        const float coef = alprev * cm;
        a0.x = fmaf(coef, p0.x, a0.x); a0.y = fmaf(coef, p0.y, a0.y); a0.z = fmaf(coef, p0.z, a0.z); a0.w = fmaf(coef, p0.w, a0.w);
        a1.x = fmaf(coef, p1.x, a1.x); a1.y = fmaf(coef, p1.y, a1.y); a1.z = fmaf(coef, p1.z, a1.z); a1.w = fmaf(coef, p1.w, a1.w);
        ah0 = fmaf(hal[t1 & 1][0] * cm, ownp, ah0);
        ah1 = fmaf(hal[t1 & 1][1] * cm, ownp, ah1);
    };
    auto step = [&](const int t, const float eraw, const float us) {
        float rb = 1.f, ib1 = 0.f;
        if (t < L - 1) {
            const f4 a = sums((t + 1) & 1);
            ib1 = 1.f / a.y;
            const float sc = finish(t + 1, a.x);
            outer(t + 1, t < L - 2 ? sc * ib2 : 0.f);         // position t + 1 has a successor
            const float *xv = sb[(t + 1) & 1];
            p0 = (f4){xv[c.s0.x], xv[c.s0.y], xv[c.s0.z], xv[c.s0.w]};
            p1 = (f4){xv[c.s1.x], xv[c.s1.y], xv[c.s1.z], xv[c.s1.w]};
            float r = fmaf(c.w0.w, p0.w, fmaf(c.w0.z, p0.z, fmaf(c.w0.y, p0.y, c.w0.x * p0.x)));
            r += fmaf(c.w1.w, p1.w, fmaf(c.w1.z, p1.z, fmaf(c.w1.y, p1.y, c.w1.x * p1.x)));
            r = i == c.hub0 ? a.z : (i == c.hub1 ? a.w : r);
            rb = fmaxf(r * ib1, eps);
        }
        const float al = __builtin_fabsf(us);
        const bool live = __builtin_bit_cast(int, us) >= 0;
        const float g = act ? al * rb : 0.f;
        const float s = act ? fmaxf(eraw, eps) * rb : 0.f;
        const float sm = live ? s : 0.f;
        sb[t & 1][i] = sm;
        f4 ps = {mq_wave_sum(g), mq_wave_sum(s), 0.f, 0.f};
        if (c.nhub > 0) ps.z = mq_wave_sum(sm * c.hw0);
        if (c.nhub > 1) ps.w = mq_wave_sum(sm * c.hw1);
        if (lane == 0) part[t & 1][w] = ps;
        if (i == c.hub0) hal[t & 1][0] = al;
        if (i == c.hub1) hal[t & 1][1] = al;
        ownp = own; own = sm;
        gprev = g; eprev = eraw; alprev = al; ib2 = ib1;
        __syncthreads();
    };
    // a ring of WQ_PF rows of E and of the parked U in flight (towards position 0): a step's registers are reloaded with
    // the rows WQ_PF positions ahead as soon as the step has taken their values; positions before the start re-read
    // row 0.  The sweep writes dE_{t+1} in step t, always behind what is read here.
    auto at = [&](int t) { return (size_t)(t > 0 ? t : 0) * q + ic; };
    float en[WQ_PF], un[WQ_PF];
#pragma unroll
    for (int u = 0; u < WQ_PF; ++u) { en[u] = Er[at(L - 1 - u)]; un[u] = o[at(L - 1 - u)]; }
    __syncthreads();                                          // hal zeroed
    for (int tb = L - 1; tb >= 0; tb -= WQ_PF) {
#pragma unroll
        for (int u = 0; u < WQ_PF; ++u) {
            const float eraw = en[u], us = un[u];
            en[u] = Er[at(tb - u - WQ_PF)];
            un[u] = o[at(tb - u - WQ_PF)];
            if (tb - u >= 0) step(tb - u, eraw, us);          // block-uniform
        }
    }
    // position 0: its dE and (L > 1) coef_0 bh_1
    const f4 a = sums(0);
    const float sc = finish(0, a.x);
    if (L > 1) outer(0, sc * ib2);
    float *ar = acc + (size_t)row * GW_ACC * NP + i;
    ar[0 * NP] = a0.x; ar[1 * NP] = a0.y; ar[2 * NP] = a0.z; ar[3 * NP] = a0.w;
    ar[4 * NP] = a1.x; ar[5 * NP] = a1.y; ar[6 * NP] = a1.z; ar[7 * NP] = a1.w;
    ar[8 * NP] = ah0;  ar[9 * NP] = ah1;
}

// dA (k,q,q) from the sequences' accumulators: one wave per (model, row i).  Every entry of the row is written: 0 where
// A[i][j] == 0, else the owner's slot summed over the model's b sequences in fp64 (lane s takes sequences s, s + 64,
// ..., then a fixed butterfly) and rounded once.
__global__ __launch_bounds__(64) void k_gw_sum(const float *__restrict__ acc, float *__restrict__ dA, int b, int q, int NP,
                                               const WqSp *__restrict__ sp) {
    const int m = blockIdx.y, i = blockIdx.x, tid = threadIdx.x;
    const WqSp &M = sp[m];
    if (!M.sparse) return;                                    // refused: k_gw_refuse writes this model's dA
    const int h = i == M.hub[0] ? 0 : (i == M.hub[1] ? 1 : -1);
    float *row = dA + ((size_t)m * q + i) * q;
    const float *am = acc + (size_t)m * b * GW_ACC * NP;
    auto total = [&](int slot, int lane) {
        double s = 0.0;
        for (int r = tid; r < b; r += 64) s += (double)am[((size_t)r * GW_ACC + slot) * NP + lane];
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        return (float)s;
    };
    if (h >= 0) {                                             // a hub's row: lane j owns h -> j
        for (int j = 0; j < q; ++j) {
            const bool has = M.hout[h][j] != 0.f;             // wave-uniform
            const float v = has ? total(WQ_SP_MAX + h, j) : 0.f;
            if (tid == 0) row[j] = v;
        }
        return;
    }
    for (int j = tid; j < q; j += 64) row[j] = 0.f;
    __syncthreads();                                          // (one wave: orders the zeros before the entries)
    for (int e = 0; e < WQ_SP_MAX; ++e) {
        if (M.bw[i][e] == 0.f) continue;                      // a pad; wave-uniform
        const float v = total(e, i);
        if (tid == 0) row[M.bsrc[i][e]] = v;
    }
}

// the refused models' outputs (NaN in every element) and the call's counter; grid (GW_REFUSE_BLOCKS, k), block 256.
// dA, dpi, dE null: the log-likelihood form.
__global__ __launch_bounds__(256) void k_gw_refuse(const WqSp *__restrict__ sp, int k, int b, int L, int q,
                                                   float *__restrict__ dA, float *__restrict__ dpi,
                                                   float *__restrict__ dE, double *__restrict__ ll,
                                                   int *__restrict__ count) {
    const int m = blockIdx.y;
    if (blockIdx.x == 0 && m == 0 && threadIdx.x == 0) {
        int n = 0;
        for (int x = 0; x < k; ++x) n += sp[x].sparse ? 0 : 1;
        *count = n;
    }
    if (sp[m].sparse) return;
    const float fnan = __builtin_bit_cast(float, 0x7fc00000u);
    const double dnan = __builtin_bit_cast(double, 0x7ff8000000000000ull);
    const size_t id = (size_t)blockIdx.x * 256 + threadIdx.x, stride = (size_t)gridDim.x * 256;
    for (size_t x = id; x < (size_t)b; x += stride) ll[(size_t)m * b + x] = dnan;
    if (!dA) return;
    const size_t nA = (size_t)q * q, nE = (size_t)b * L * q;
    for (size_t x = id; x < nA; x += stride) dA[(size_t)m * nA + x] = fnan;
    for (size_t x = id; x < (size_t)q; x += stride) dpi[(size_t)m * q + x] = fnan;
    for (size_t x = id; x < nE; x += stride) dE[(size_t)m * nE + x] = fnan;
}

// ---- host side
struct GwPlan { int NP; size_t o_ll, o_sp, o_count, o_acc, total; };
static int make_gwplan(int k, int b, int L, int q, GwPlan *p) {
    if (k < 1 || b < 1 || L < 1 || q < 1) return HMM_ERR_BAD_SHAPE;
    if (q < WQ_MIN || q > WQ_MAX) return HMM_ERR_Q_UNSUPPORTED;
    p->NP = (q + 63) / 64 * 64;
    size_t off = 0;
    p->o_ll = off;    off = align_up(off + (size_t)k * b * sizeof(double));
    p->o_sp = off;    off = align_up(off + (size_t)k * sizeof(WqSp));
    p->o_count = off; off = align_up(off + sizeof(int));
    p->o_acc = off;   off = align_up(off + (size_t)k * b * GW_ACC * p->NP * sizeof(float));
    p->total = off;
    return HMM_OK;
}

extern "C" {

int hmm_loglik_grad_walk_min_states(void) { return WQ_MIN; }
int hmm_loglik_grad_walk_max_states(void) { return WQ_MAX; }

size_t hmm_loglik_grad_walk_workspace_bytes(int k, int b, int L, int q) {
    GwPlan p;
    return make_gwplan(k, b, L, q, &p) ? 0 : p.total;
}

// 1 where this call measured at least 1.25x faster than hmm_loglik_grad_large at its default route (DESIGN §11d;
// tools/experiments/loglik_grad_walk_time.py, profiles/loglik_grad_walk.json); 0 where nothing was measured.  Measured
// on one MI355X at L = 10 000, one model, 1 / 32 / 1024 sequences: 3.2x at 71 states and 4.2 .. 7.5x at 127 (against
// the dense walk), 19 .. 27x at 253 (against the per-position GEMMs) — every cell pays, so the rule is the measured
// range itself, as for hmm_posterior_walk_pays: up to GW_PAYS_SEQS sequences in the call.  More sequences were not
// measured.  L does not enter: both evaluations cost per position.  Only models inside the sparse rule were measured
// (others are refused).
#define GW_PAYS_SEQS 1024
int hmm_loglik_grad_walk_pays(int k, int b, int L, int q) {
    GwPlan p;
    if (make_gwplan(k, b, L, q, &p)) return 0;
    return (long long)k * b <= GW_PAYS_SEQS ? 1 : 0;
}

long long hmm_loglik_grad_walk_refused(int k, int b, int L, int q, const void *workspace, size_t workspace_bytes) {
    GwPlan p;
    int rc = make_gwplan(k, b, L, q, &p);
    if (rc) return rc;
    if (!workspace) return HMM_ERR_NULL_POINTER;
    if (workspace_bytes < p.total) return HMM_ERR_WORKSPACE;
    int v = 0;
    if (hipMemcpy(&v, ws_at<int>(workspace, p.o_count), sizeof(int), hipMemcpyDeviceToHost) != hipSuccess)
        return HMM_ERR_LAUNCH;
    return v;
}

int hmm_loglik_grad_walk(const float *A, const float *pi, const float *E, int k, int b, int L, int q, float eps,
                         const float *grad_loglik, float *dA, float *dpi, float *dE, double *loglik, void *workspace,
                         size_t workspace_bytes, void *stream) {
    GwPlan p;
    int rc = make_gwplan(k, b, L, q, &p);
    if (rc) return rc;
    const int ngrad = (dA ? 1 : 0) + (dpi ? 1 : 0) + (dE ? 1 : 0);
    if (!A || !pi || !E || !workspace || (ngrad != 0 && ngrad != 3) || (ngrad == 0 && !loglik))
        return HMM_ERR_NULL_POINTER;
    if ((rc = check_eps(eps))) return rc;
    if ((rc = check_ws(p.total, workspace, workspace_bytes))) return rc;
    hipStream_t st = (hipStream_t)stream;
    WqSp *sp = ws_at<WqSp>(workspace, p.o_sp);
    const WqSp *csp = sp;
    double *ll = ws_at<double>(workspace, p.o_ll);
    float *acc = ws_at<float>(workspace, p.o_acc);
    const dim3 grid((unsigned)((size_t)k * b)), blk((unsigned)p.NP);
    launch(k_wq_prep, dim3(k), dim3(WQ_MAX), 0, st, A, sp, q, 0);
    if (ngrad) {
        launch(k_gw_fwd<true>, grid, blk, 0, st, pi, E, b, L, q, eps, dE, ll, csp);
        launch(k_gw_bwd, grid, blk, 0, st, E, b, L, q, eps, grad_loglik, dE, acc, csp);
        launch(k_gw_sum, dim3(q, k), dim3(64), 0, st, (const float *)acc, dA, b, q, p.NP, csp);
        launch(k_mq_grad_pi, dim3(q, k), dim3(64), 0, st, pi, E, dE, b, L, q, eps, dpi);
    } else {
        launch(k_gw_fwd<false>, grid, blk, 0, st, pi, E, b, L, q, eps, (float *)nullptr, ll, csp);
    }
    launch(k_gw_refuse, dim3(GW_REFUSE_BLOCKS, k), dim3(256), 0, st, csp, k, b, L, q, dA, dpi, dE, ll,
           ws_at<int>(workspace, p.o_count));
    if (loglik) launch(k_copy_loglik, dim3((k * b + 255) / 256), dim3(256), 0, st, (const double *)ll, loglik, k * b);
    return check_launch();
}

}  // extern "C"
