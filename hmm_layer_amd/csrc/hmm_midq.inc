// hmm_midq.inc — forward / backward / posterior for 16 < q <= 64 states (e.g. the 29-state two-copy
// gene model), included by hmm_engine.hip.
//
// A scan over q x q operators costs q^3 per position and the batched-GEMM path (hmm_largeq.inc) needs
// two launches per position, which for q of a few dozen is all launch latency (~12 us per position:
// over a second for L = 1e5).  In this range a whole sequence fits ONE wave: lane j owns state j, keeps
// column j of A (forward) or row j (backward) in registers, and the previous vector reaches every
// lane through v_readlane broadcasts — the reference's per-step matmul
// (hmm_layer/gene_pred_hmm_transitioner.py:122-125) is q fma's per lane.  One persistent kernel per
// direction walks the sequence with the cell's exact step semantics (hmm_layer/MsaHmmCell.py:73-106:
// both clamps, emission product, row sum, normalise, log of the normaliser in fp64); sequences are
// independent waves.  The posterior keeps alpha_hat in the output tensor on the way forward and
// overwrites it with gamma on the way back, as the large-q path does.

#define MQ_MAX 64
#ifndef MQ_PF
#define MQ_PF 8            // emission rows in flight
#endif

// sum over the 64 lanes, result in every lane: DPP all-reduce inside each 16-lane row, then the
// permlane butterfly across the four rows — VALU only (a __shfl_xor tree goes through the LDS
// crossbar six times per sum and dominated the step: 0.47 -> 0.2x us per position)
__device__ __forceinline__ float mq_wave_sum(float v) { return col_sum(row_sum_f(v)); }
// the same sum, same order of additions, with the row stages as ONE instruction each (the shuffle as the add's
// operand modifier; the intrinsic form costs a copy, a v_mov_dpp and the add): the sparse steps are issue-bound
__device__ __forceinline__ float mq_wave_sum_fast(float v) {
    float a, b, c, d;
    asm("s_nop 1\n\tv_add_f32_dpp %0, %1, %1 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf" : "=&v"(a) : "v"(v));
    asm("s_nop 1\n\tv_add_f32_dpp %0, %1, %1 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf" : "=&v"(b) : "v"(a));
    asm("s_nop 1\n\tv_add_f32_dpp %0, %1, %1 row_half_mirror row_mask:0xf bank_mask:0xf" : "=&v"(c) : "v"(b));
    asm("s_nop 1\n\tv_add_f32_dpp %0, %1, %1 row_mirror row_mask:0xf bank_mask:0xf" : "=&v"(d) : "v"(c));
    return col_sum(d);
}
#define MQ_LN2 0.6931471805599453
// the sparse steps (D != 0) take the one-instruction row stages and accumulate the normalisers' log2 (one
// v_log_f32; S is a normal number), scaled by ln 2 where the sum is used; the dense steps are as they were
template <int D> __device__ __forceinline__ float mq_sum(float v) { return D ? mq_wave_sum_fast(v) : mq_wave_sum(v); }
template <int D> __device__ __forceinline__ float mq_logacc(float S) { return D ? __builtin_amdgcn_logf(S) : __logf(S); }
template <int D> __device__ __forceinline__ double mq_logscale() { return D ? MQ_LN2 : 1.0; }

// ---- decoded output for 17..64 states (hmm_posterior_decode_mid): the output policy of the posterior kernels of this
// file (k_mq_posterior2) and of the chunked scan (backward<NT, 0> in hmm_scan_rows.inc).  NoDecode (hmm_engine.hip)
// writes the gamma rows; DecodeMid collapses every gamma row, staged in LDS, to (class with the largest posterior, that
// posterior): 1 + 4 bytes per position instead of 4 q.  A 16 x 64 weight table does not fit the argument segment next
// to the other arguments, so the class table travels as sixteen 64-bit membership masks by value (a captured graph
// keeps its table) and every block expands it once into a 0 / 1 weight per (class, state) in LDS (mid_weights).  A
// class sum is then broadcast LDS reads and fma(v, w, sum) over ALL states in increasing index: fma(v, 1, sum) is
// sum + v rounded once and fma(v, 0, sum) is sum, the bits of adding the members alone (DESIGN 4).
struct alignas(8) DecodeMid {
    static constexpr bool on = true;
    unsigned long long mask[QP];     // bit s of mask[c]: state s belongs to class c
    unsigned char *label;            // (k,b,L)
    float *conf;                     // (k,b,L) or null
    int ncls;                        // number of classes; 0: the identity map (no sums)
};
#define MID_WT_FLOATS (QP * MQ_MAX)

// wt[c * 64 + s] for the whole block; every thread of the block calls this before any of them leaves
__device__ __forceinline__ void mid_weights(const DecodeMid &d, float *wt) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
#pragma unroll
    for (int c = 0; c < QP; ++c)                                           // (constant indices: the masks stay arguments)
        if (c % nw == wv) wt[c * MQ_MAX + lane] = ((d.mask[c] >> lane) & 1ull) ? 1.f : 0.f;
    __syncthreads();
}

// One staged gamma row (q floats in LDS) -> label[at], conf[at]: the ONE collapse routine of both kernels.  W: the row
// width the weights are walked over (a multiple of PIECE; states from q on read as 0 and weigh 0); PIECE: how many
// values of the row are in registers at a time — the whole row where the registers are there (each value is read
// once), 16 where they are not (the row is read again for every class).  Identity map: the largest entry and its
// lowest index, nothing summed.
template <int W, int PIECE>
__device__ __forceinline__ void collapse_row(const float *row, int q, const DecodeMid &d, const float *wt, long long at) {
    static_assert(W % PIECE == 0 && PIECE % 4 == 0 && W <= MQ_MAX, "whole pieces of a row of up to 64 states");
    float best = row[0];
    int lab = 0;
    if (d.ncls == 0) {
#pragma unroll 4
        for (int s = 1; s < q; ++s) {
            const float v = row[s];
            if (v > best) { best = v; lab = s; }                          // strict: the lowest index wins a tie
        }
    } else {
        float v[PIECE];
        auto load = [&](int s0) {
#pragma unroll
            for (int u = 0; u < PIECE; ++u) v[u] = s0 + u < q ? row[s0 + u] : 0.f;
        };
        if constexpr (PIECE == W) load(0);
#pragma unroll 1
        for (int cl = 0; cl < d.ncls; ++cl) {
            float sum = 0.f;                                               // states in increasing index
#pragma unroll
            for (int s0 = 0; s0 < W; s0 += PIECE) {
                if (PIECE != W && s0 >= q) break;                          // (uniform)
                if constexpr (PIECE != W) load(s0);
                const f4 *w4 = reinterpret_cast<const f4 *>(wt + cl * MQ_MAX + s0);
#pragma unroll
                for (int u = 0; u < PIECE / 4; ++u) {
                    const f4 w = w4[u];
                    sum = __builtin_fmaf(v[4 * u + 0], w.x, sum);
                    sum = __builtin_fmaf(v[4 * u + 1], w.y, sum);
                    sum = __builtin_fmaf(v[4 * u + 2], w.z, sum);
                    sum = __builtin_fmaf(v[4 * u + 3], w.w, sum);
                }
            }
            if (cl == 0 || sum > best) { best = sum; lab = cl; }          // strict: the lowest class wins a tie
        }
    }
    __builtin_nontemporal_store((unsigned char)lab, d.label + at);
    if (d.conf) __builtin_nontemporal_store(best, d.conf + at);
}

// Row prefetch of the one-wave-per-sequence kernels: MQ_PF rows of a (L, q) slab in flight, one dword per lane and
// row, through a buffer descriptor that covers exactly the rows wanted — rows outside [t1 bounds] fall outside
// the descriptor and read 0, so there is NO branch around the loads.  (With the loads under `if (t + MQ_PF < L)` the
// compiler's wait-count pass gave up: s_waitcnt vmcnt(0) every step, a memory latency per position.)
// Idle lanes (>= q) read their neighbours' values; every caller masks them.
struct MqRows {
    const float *base;        // row 0 of the sequence's slab
    int q, rowb, voff;
    __device__ __forceinline__ MqRows(const float *b_, int q_, int lane) : base(b_), q(q_), rowb(q_ * 4), voff(lane * 4) {}
    // rows t0, t0 + 1, ... (those below t1)
    __device__ __forceinline__ void up(int t0, int t1, float (&r)[MQ_PF]) const {
        int n = t1 - t0;
        n = n < 0 ? 0 : (n > MQ_PF ? MQ_PF : n);
        const __amdgpu_buffer_rsrc_t rs = make_rsrc(base + (long long)t0 * q, (unsigned long long)(n * rowb));
#pragma unroll
        for (int u = 0; u < MQ_PF; ++u)
            r[u] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, voff + u * rowb, 0, 0));
    }
    // rows t0, t0 - 1, ... (those at or above t1)
    __device__ __forceinline__ void down(int t0, int t1, float (&r)[MQ_PF]) const {
        int lo = t0 - MQ_PF + 1;
        lo = lo < t1 ? t1 : lo;
        int n = t0 - lo + 1;
        n = n < 0 ? 0 : n;
        const __amdgpu_buffer_rsrc_t rs = make_rsrc(base + (long long)lo * q, (unsigned long long)(n * rowb));
#pragma unroll
        for (int u = 0; u < MQ_PF; ++u)                     // a row below lo: negative offset = out of range
            r[u] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, voff + (t0 - u - lo) * rowb, 0, 0));
    }
};
// nothing in flight when a prefetching loop is entered: otherwise the wait counts at the loop head are those of
// the way in, where fewer operations follow the rows just requested (hmm_viterbi.inc, k_mq_viterbi)
__device__ __forceinline__ void mq_drain() { __builtin_amdgcn_s_waitcnt(0x0F70); }

// ---- the dense mat-vec of these kernels: sum_i c[i] * x[lane i] for this lane's QB coefficients.  Each 16-lane row
// of x is first replicated into every row (one ds_bpermute per row), then every term is ONE instruction,
// v_fmac_f32 with the DPP row broadcast as its operand modifier (the v_readlane + v_fma pair it replaces was two).
// Same four accumulators and order of additions as before: identical results.
template <int QB> struct MqDense {
    float xr[QB / 16];                                       // row r of the vector, in every row
    __device__ __forceinline__ void spread(float x, int lane) {
        const int xi = __builtin_bit_cast(int, x);
#pragma unroll
        for (int r = 0; r < QB / 16; ++r)
            xr[r] = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute((16 * r + (lane & 15)) * 4, xi));
    }
    // acc += x[16 R + N] * c in ONE instruction: the row broadcast as the DPP modifier of the fma's first operand (the
    // compiler keeps v_mov_b32_dpp + v_fma apart).  Inline asm, so the "VALU write -> DPP read" hazard of xr is
    // covered by hand: the first of a run of these waits two cycles.
    template <int R, int N> __device__ __forceinline__ void fmac(float &acc, float c) const {
        if (N == 0)
            asm volatile("s_nop 1\n\tv_fmac_f32_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(xr[R]), "v"(c), "n"(N));
        else
            asm volatile("v_fmac_f32_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(xr[R]), "v"(c), "n"(N));
    }
};
template <int QB, int I> struct MqDenseLoop {
    static __device__ __forceinline__ void dot(const MqDense<QB> &d, const float (&c)[QB], float (&r)[4]) {
        d.template fmac<I / 16, I % 16>(r[I & 3], c[I]);
        MqDenseLoop<QB, I + 1>::dot(d, c, r);
    }
    // g[i] += coef * x[i] (the gradient kernel's sums of xi)
    static __device__ __forceinline__ void outer(const MqDense<QB> &d, float coef, float (&g)[QB]) {
        d.template fmac<I / 16, I % 16>(g[I], coef);
        MqDenseLoop<QB, I + 1>::outer(d, coef, g);
    }
};
template <int QB> struct MqDenseLoop<QB, QB> {
    static __device__ __forceinline__ void dot(const MqDense<QB> &, const float (&)[QB], float (&)[4]) {}
    static __device__ __forceinline__ void outer(const MqDense<QB> &, float, float (&)[QB]) {}
};
template <int QB>
__device__ __forceinline__ float mq_dense_dot(const float (&c)[QB], float x, int lane) {
    MqDense<QB> d;
    d.spread(x, lane);
    float r[4] = {0.f, 0.f, 0.f, 0.f};
    MqDenseLoop<QB, 0>::dot(d, c, r);
    return (r[0] + r[1]) + (r[2] + r[3]);
}

// ---- sparse models.  The multi-copy gene models of this range (29 / 43 / 57 states) have at most 3 / 4 / 5
// transitions into a state and 4 out of one; the dense step spends q v_readlane + q fma on a mat-vec that has
// that many non-zero terms.  k_mq_sp_prep lists, per model and on the device, every state's predecessors (column of
// A, for the forward recursion) and successors (row, for the backward one) with their weights; if no state has
// more than MQ_SP_MAX of either, lane j gathers just those with ds_bpermute (D = 4 or 8 gathers, pads weigh 0).
// Entries that are exactly 0 contribute nothing to the dense sums either: same mathematics, different rounding
// order (compared with the oracle at the usual tolerances).
// The sparse steps also carry the vector UNNORMALISED (u_t = E'_t max(R_t, eps)) next to 1 / S_t: the wave-wide sum
// is then formed while the next step's gathers are in flight, and the dependent chain of a step is
// gather -> D fma -> scale -> clamp -> emission.
#define MQ_SP_MAX 8
struct MqSp {
    int mode_f, mode_b, mode_p, pad;  // 0: dense; else 4 or 8 gathers (forward | backward | both, for the two-wave posterior)
    int fsrc[64][MQ_SP_MAX];          // predecessors of state j (lane j), pads: 0 with weight 0
    float fw[64][MQ_SP_MAX];
    int bsrc[64][MQ_SP_MAX];          // successors of state i
    float bw[64][MQ_SP_MAX];
};

static_assert(sizeof(MqSp) == LQ_SP_BYTES, "LqPlan reserves LQ_SP_BYTES per model");

__global__ __launch_bounds__(64) void k_mq_sp_prep(const float *__restrict__ A, MqSp *__restrict__ sp, int q,
                                                   int force_dense) {
    const int m = blockIdx.x, j = threadIdx.x;
    const float *Am = A + (size_t)m * q * q;
    MqSp &M = sp[m];
    int nf = 0, nb = 0;
    if (j < q) {
        for (int i = 0; i < q; ++i) {
            const float a = Am[(size_t)i * q + j];
            if (a != 0.f) { if (nf < MQ_SP_MAX) { M.fsrc[j][nf] = i; M.fw[j][nf] = a; } ++nf; }
            const float c = Am[(size_t)j * q + i];
            if (c != 0.f) { if (nb < MQ_SP_MAX) { M.bsrc[j][nb] = i; M.bw[j][nb] = c; } ++nb; }
        }
    }
    for (int e = nf < MQ_SP_MAX ? nf : MQ_SP_MAX; e < MQ_SP_MAX; ++e) { M.fsrc[j][e] = 0; M.fw[j][e] = 0.f; }
    for (int e = nb < MQ_SP_MAX ? nb : MQ_SP_MAX; e < MQ_SP_MAX; ++e) { M.bsrc[j][e] = 0; M.bw[j][e] = 0.f; }
    int df = nf, db = nb;
    for (int o = 32; o > 0; o >>= 1) { df = max(df, __shfl_xor(df, o)); db = max(db, __shfl_xor(db, o)); }
    if (j == 0) {
        const int mf = (force_dense || df > MQ_SP_MAX) ? 0 : (df <= 4 ? 4 : 8);
        const int mb = (force_dense || db > MQ_SP_MAX) ? 0 : (db <= 4 ? 4 : 8);
        M.mode_f = mf; M.mode_b = mb;
        M.mode_p = (mf && mb) ? max(mf, mb) : 0;
        M.pad = 0;
    }
}

// this lane's D sources (as ds_bpermute byte addresses) and weights, held as vector VALUES (a register array
// indexed under selects ends up in scratch, see k_mq_viterbi)
template <int D> struct MqSpLane { i4 s0, s1; f4 w0, w1; };
template <int D>
__device__ __forceinline__ MqSpLane<D> mq_sp_lane(const int (*src)[MQ_SP_MAX], const float (*w)[MQ_SP_MAX], int lane) {
    MqSpLane<D> l;
    l.s0 = *reinterpret_cast<const i4 *>(&src[lane][0]) * 4;
    l.w0 = *reinterpret_cast<const f4 *>(&w[lane][0]);
    l.s1 = l.s0; l.w1 = l.w0;
    if constexpr (D == 8) {
        l.s1 = *reinterpret_cast<const i4 *>(&src[lane][4]) * 4;
        l.w1 = *reinterpret_cast<const f4 *>(&w[lane][4]);
    }
    return l;
}
// v[src_x] for this lane's D sources: issued as soon as v exists, consumed a step later (mq_sp_reduce), so that the
// LDS round trip runs under the wave-wide sum of the same step
template <int D> struct MqGath { f4 a, b; };
template <int D>
__device__ __forceinline__ MqGath<D> mq_sp_gather(const MqSpLane<D> &l, float v) {
    const int vi = __builtin_bit_cast(int, v);
    MqGath<D> g;
    g.a.x = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(l.s0.x, vi));
    g.a.y = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(l.s0.y, vi));
    g.a.z = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(l.s0.z, vi));
    g.a.w = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(l.s0.w, vi));
    g.b = g.a;
    if constexpr (D == 8) {
        g.b.x = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(l.s1.x, vi));
        g.b.y = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(l.s1.y, vi));
        g.b.z = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(l.s1.z, vi));
        g.b.w = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(l.s1.w, vi));
    }
    return g;
}
// sum_x w_x * v[src_x]
template <int D>
__device__ __forceinline__ float mq_sp_reduce(const MqSpLane<D> &l, const MqGath<D> &g) {
    float r = fmaf(l.w0.w, g.a.w, fmaf(l.w0.z, g.a.z, fmaf(l.w0.y, g.a.y, l.w0.x * g.a.x)));
    if constexpr (D == 8) r += fmaf(l.w1.w, g.b.w, fmaf(l.w1.z, g.b.z, fmaf(l.w1.y, g.b.y, l.w1.x * g.b.x)));
    return r;
}
// which instantiation serves model m: the dense one (D = 0) everything when there is no table
template <int D>
__device__ __forceinline__ bool mq_sp_mine(const MqSp *sp, int m, int which) {     // which: 0 forward, 1 backward, 2 both
    if (!sp) return D == 0;
    const int mode = which == 0 ? sp[m].mode_f : (which == 1 ? sp[m].mode_b : sp[m].mode_p);
    return mode == D;
}

// out_alpha (row stride L*q) receives alpha_hat_t, log_alpha (same layout) log alpha_t; either may be null
// SIGNED: alpha_hat is stored with the sign bit set where the cell's clamp of the predicted state
// was active ((x A)[j] <= eps, MsaHmmCell.py:88) — what the gradient kernel needs to know
template <int QB, bool SIGNED, int D = 0>
__device__ __forceinline__ void mq_forward_body(const float *__restrict__ A, const float *__restrict__ pi,
                                                const float *__restrict__ E, int b, int L, int q, float eps,
                                                float *__restrict__ out_alpha, float *__restrict__ log_alpha,
                                                double *__restrict__ ll, float *__restrict__ Sout,
                                                const int *__restrict__ need = nullptr, const MqSp *__restrict__ sp = nullptr) {
    const int row = blockIdx.x, m = row / b, j = threadIdx.x & 63;
    if (need && !need[row]) return;                          // (17..32 states) served by the chunked scan
    if (!mq_sp_mine<D>(sp, m, 0)) return;                    // the other instantiation has this model
    const bool act = j < q;
    const float *Am = A + (size_t)m * q * q;
    constexpr int NA = D ? 16 : QB;                          // (sparse instantiations: the dense step is dead code)
    float acol[NA];
    MqSpLane<D ? D : 4> sl;
    if constexpr (D == 0) {
#pragma unroll
        for (int i = 0; i < QB; ++i) acol[i] = (act && i < q) ? Am[(size_t)i * q + j] : 0.f;
    } else {
        sl = mq_sp_lane<D>(sp[m].fsrc, sp[m].fw, j);
    }
    const float *Er = E + (size_t)row * L * q;
    const size_t obase = (size_t)row * L * q;
    float x = act ? pi[(size_t)m * q + j] : 0.f;
    float inv = 1.f;                                        // sparse step: x is unnormalised, inv = 1 / its sum
    MqGath<D ? D : 4> gx = {};                              // ... and gx its gathered predecessors
    double lacc = 0.0;
    const MqRows rows(Er, q, j);
    float en[MQ_PF];
    rows.up(0, L, en);
    auto step = [&](int t, float eraw) {
        const float e = fmaxf(eraw, eps);
        if constexpr (D != 0) {
            const float r = mq_sp_reduce<D>(sl, gx);
            const float R = t > 0 ? r * inv : x;
            const float sf = act ? e * fmaxf(R, eps) : 0.f;
            gx = mq_sp_gather<D>(sl, sf);                    // for the next step, in flight under the sum
            const float S = mq_wave_sum_fast(sf);
            inv = __builtin_amdgcn_rcpf(S);
            x = sf;
            // log2, scaled at the end (S is a normal number: >= eps^2 with eps >= HMM_EPS_MIN)
            lacc += (double)__builtin_amdgcn_logf(S);
            if (Sout && j == 0) Sout[(size_t)row * L + t] = S;
            if (act) {
                const float xn = sf * inv;
                if (out_alpha) out_alpha[obase + (size_t)t * q + j] = (SIGNED && !(R > eps)) ? -xn : xn;
                if (log_alpha) log_alpha[obase + (size_t)t * q + j] = __logf(xn) + (float)(lacc * MQ_LN2);
            }
            return;
        }
        float R = x;
        if (t > 0) R = mq_dense_dot<NA>(acol, x, j);
        const float sf = act ? e * fmaxf(R, eps) : 0.f;
        const float S = mq_wave_sum(sf);
        x = sf * __builtin_amdgcn_rcpf(S);
        lacc += (double)__logf(S);
        if (Sout && j == 0) Sout[(size_t)row * L + t] = S;
        if (act) {
            if (out_alpha) out_alpha[obase + (size_t)t * q + j] = (SIGNED && !(R > eps)) ? -x : x;
            if (log_alpha) log_alpha[obase + (size_t)t * q + j] = __logf(x) + (float)lacc;
        }
    };
    mq_drain();
    int tb = 0;
    for (; tb + MQ_PF <= L; tb += MQ_PF) {                  // whole blocks: no branch inside
        float cur[MQ_PF];
#pragma unroll
        for (int u = 0; u < MQ_PF; ++u) cur[u] = en[u];
        rows.up(tb + MQ_PF, L, en);
#pragma unroll
        for (int u = 0; u < MQ_PF; ++u) step(tb + u, cur[u]);
    }
#pragma unroll
    for (int u = 0; u < MQ_PF; ++u)
        if (tb + u < L) step(tb + u, en[u]);                // wave-uniform
    if (j == 0) ll[row] = D ? lacc * MQ_LN2 : lacc;
}

template <int QB, bool SIGNED = false, int D = 0>
__global__ __launch_bounds__(64) void k_mq_forward(const float *__restrict__ A, const float *__restrict__ pi,
                                                   const float *__restrict__ E, int b, int L, int q, float eps,
                                                   float *__restrict__ out_alpha, float *__restrict__ log_alpha,
                                                   double *__restrict__ ll, float *__restrict__ Sout = nullptr,
                                                   const int *__restrict__ need = nullptr,
                                                   const MqSp *__restrict__ sp = nullptr) {
    mq_forward_body<QB, SIGNED, D>(A, pi, E, b, L, q, eps, out_alpha, log_alpha, ll, Sout, need, sp);
}

// mode 0/1/2: out_t = alpha_hat_t * Rb / sum (prob | log | log + loglik), alpha_hat_t read from out_t;
// mode 3: out_t = log Rb + lscale (log beta).  Rb = init ? 1 : max(A b_hat, eps).
template <int QB, int D = 0>
__global__ __launch_bounds__(64) void k_mq_backward(const float *__restrict__ A, const float *__restrict__ E,
                                                    int b, int L, int q, float eps, float *__restrict__ out,
                                                    const double *__restrict__ loglik, int mode,
                                                    const int *__restrict__ need = nullptr,
                                                    const MqSp *__restrict__ sp = nullptr) {
    const int row = blockIdx.x, m = row / b, i = threadIdx.x;
    if (need && !need[row]) return;
    if (!mq_sp_mine<D>(sp, m, 1)) return;
    const bool act = i < q;
    const float *Am = A + (size_t)m * q * q;
    constexpr int NA = D ? 16 : QB;                          // (sparse instantiations: the dense step is dead code)
    float arow[NA];
    MqSpLane<D ? D : 4> sl;
    if constexpr (D == 0) {
#pragma unroll
        for (int jj = 0; jj < QB; ++jj) arow[jj] = (act && jj < q) ? Am[(size_t)i * q + jj] : 0.f;
    } else {
        sl = mq_sp_lane<D>(sp[m].bsrc, sp[m].bw, i);
    }
    const float *Er = E + (size_t)row * L * q;
    float *o = out + (size_t)row * L * q;
    const float llf = (mode == 2) ? (float)loglik[row] : 0.f;
    float bh = 0.f;
    double ls = 0.0;
    const MqRows rows(Er, q, i), arows(o, q, i);
    float en[MQ_PF], an[MQ_PF];
    const int noa = mode != 3 ? 0 : L;                     // log beta: alpha_hat is not read (an empty descriptor, no branch)
    rows.down(L - 1, 0, en);
    arows.down(L - 1, noa, an);
    float binv = 1.f;                                       // sparse step: bh is unnormalised, binv = 1 / its sum
    MqGath<D ? D : 4> gb = {};                              // ... and gb its gathered successors
    auto step = [&](int t, float eraw, float al) {
        const float e = fmaxf(eraw, eps);
        float rb = 1.f;
        if constexpr (D != 0) {
            const float r = mq_sp_reduce<D>(sl, gb);
            rb = t < L - 1 ? fmaxf(r * binv, eps) : 1.f;
            gb = mq_sp_gather<D>(sl, act ? e * rb : 0.f);   // for the next step, in flight under the sums below
        } else if (t < L - 1) {
            rb = fmaxf(mq_dense_dot<NA>(arow, bh, i), eps);
        }
        float v;
        if (mode == 3) {
            v = __logf(rb) + (float)(ls * mq_logscale<D>());
        } else {
            const float g = act ? al * rb : 0.f;
            const float Sg = mq_sum<D>(g);
            v = (mode == 0) ? g * __builtin_amdgcn_rcpf(Sg) : __logf(g) - (__logf(Sg) - llf);
        }
        if (act) o[(size_t)t * q + i] = v;
        const float sb = act ? e * rb : 0.f;
        const float Sb = mq_sum<D>(sb);
        if constexpr (D != 0) { bh = sb; binv = __builtin_amdgcn_rcpf(Sb); }
        else bh = sb * __builtin_amdgcn_rcpf(Sb);
        ls += (double)mq_logacc<D>(Sb);
    };
    mq_drain();
    int tb = L - 1;
    for (; tb - MQ_PF + 1 >= 0; tb -= MQ_PF) {              // whole blocks: no branch inside
        float ce[MQ_PF], ca[MQ_PF];
#pragma unroll
        for (int u = 0; u < MQ_PF; ++u) { ce[u] = en[u]; ca[u] = an[u]; }
        rows.down(tb - MQ_PF, 0, en);
        arows.down(tb - MQ_PF, noa, an);
#pragma unroll
        for (int u = 0; u < MQ_PF; ++u) step(tb - u, ce[u], ca[u]);
    }
#pragma unroll
    for (int u = 0; u < MQ_PF; ++u)
        if (tb - u >= 0) step(tb - u, en[u], an[u]);        // wave-uniform
}

// Posterior (modes 0 / 1) with the two sweeps side by side: wave 0 walks forward, wave 1 backward, they
// meet at m = L / 2.  Before the meeting point each parks its own vector in `out` (alpha_hat_t for
// t < m, Rb_t for t >= m); after one barrier each finds the other's vector there and overwrites it
// with gamma_t.  Same arithmetic as k_mq_forward + k_mq_backward, half the latency (the sweeps are
// dependent chains: 105 -> ~55 ms for q = 29, b = 1024, L = 1e5).
//
// DEC = DecodeMid (hmm_posterior_decode_mid, mode 0): there is no `out`.  The vectors are parked in `out` all the same
// — the caller hands the workspace's parking region, k b L q floats addressed like the output —, and in place of the
// gamma store each wave stages its rows in a wave-private LDS ring of MQ_RING rows (lds: the block's weight table,
// then the two rings; rows q | 1 floats apart, so that the lanes of a drain are on distinct banks).  The ring fills
// by whole blocks of MQ_PF steps from empty, so it is full exactly after MQ_RING / MQ_PF blocks: it is drained there,
// BETWEEN two blocks (where the fewest registers are live), with all MQ_RING rows in it, and once more at the end
// with the 0 .. MQ_RING - 1 rows that are left (the last whole blocks and the ragged tail of up to MQ_PF - 1 steps).
// In a drain lane r collapses row r (collapse_row).  Wave 0's rows ascend from L / 2, wave 1's descend from
// L / 2 - 1.  Every instruction up to the gamma value is shared with the NoDecode form.
#define MQ_RING 64
static_assert(MQ_RING % MQ_PF == 0, "the ring is full after a whole number of step blocks");
template <int QB, int D, class DEC>
__device__ __forceinline__ void mq_posterior2_body(const float *__restrict__ A, const float *__restrict__ pi,
                                                   const float *__restrict__ E, int b, int L, int q, float eps,
                                                   float *__restrict__ out, double *__restrict__ ll, int mode,
                                                   const int *__restrict__ need, const MqSp *__restrict__ sp,
                                                   const DEC &dec, float *lds) {
    const int row = blockIdx.x, m = row / b, j = threadIdx.x & 63;
    if (need && !need[row]) return;                          // block-uniform: before the barriers
    if (!mq_sp_mine<D>(sp, m, 2)) return;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int rstride = q | 1;
    float *ring = DEC::on ? lds + MID_WT_FLOATS + wv * MQ_RING * rstride : nullptr;
    int cnt = 0, tfirst = 0;                                 // rows in the ring, the position of its row 0
    auto drain = [&]() {
        if constexpr (DEC::on) {
            __builtin_amdgcn_wave_barrier();
            if (j < cnt)
                collapse_row<MQ_MAX, 4>(ring + j * rstride, q, dec, lds,
                                         (long long)row * L + (wv == 0 ? tfirst + j : tfirst - j));
            __builtin_amdgcn_wave_barrier();
            cnt = 0;
        }
    };
    const bool act = j < q;
    const float *Am = A + (size_t)m * q * q;
    const float *Er = E + (size_t)row * L * q;
    float *o = out + (size_t)row * L * q;
    const int mid = L / 2;
    constexpr int NA = D ? 16 : QB;                          // (sparse instantiations: the dense step is dead code)
    float av[NA];                                            // column j of A (forward wave) or row j (backward wave)
    MqSpLane<D ? D : 4> sl;
    if constexpr (D == 0) {
#pragma unroll
        for (int i = 0; i < QB; ++i) av[i] = (act && i < q) ? (wv == 0 ? Am[(size_t)i * q + j] : Am[(size_t)j * q + i]) : 0.f;
    } else {
        sl = wv == 0 ? mq_sp_lane<D>(sp[m].fsrc, sp[m].fw, j) : mq_sp_lane<D>(sp[m].bsrc, sp[m].bw, j);
    }
    float vinv = 1.f;                                        // sparse: the carried vector is unnormalised, vinv = 1 / its sum
    MqGath<D ? D : 4> gv = {};                               // ... and gv its gathered neighbours (issued when it was formed)
    auto matvec = [&](float v) {
        if constexpr (D != 0) return mq_sp_reduce<D>(sl, gv) * vinv;
        return mq_dense_dot<NA>(av, v, j);
    };
    auto emit = [&](float al, float rb, int t) {             // gamma_t from alpha_hat_t and Rb_t
        const float g = act ? al * rb : 0.f;
        const float Sg = mq_sum<D>(g);
        if constexpr (DEC::on) {
            if (cnt == 0) tfirst = t;
            if (act) ring[cnt * rstride + j] = g * __builtin_amdgcn_rcpf(Sg);
            ++cnt;
        } else {
            const float v = (mode == 0) ? g * __builtin_amdgcn_rcpf(Sg) : __logf(g) - __logf(Sg);
            if (act) o[(size_t)t * q + j] = v;
        }
    };
    if (wv == 0) {
        float x = act ? pi[(size_t)m * q + j] : 0.f;
        double lacc = 0.0;
        const MqRows rows(Er, q, j), orows(o, q, j);
        for (int phase = 0; phase < 2; ++phase) {
            const int t0 = phase ? mid : 0, t1 = phase ? L : mid;
            const int tr = phase ? t1 : 0;                  // phase 0 reads nothing from `out` (empty descriptor)
            float en[MQ_PF], rn[MQ_PF];
            rows.up(t0, t1, en);
            orows.up(t0, tr, rn);
            auto step = [&](int t, float eraw, float rbv) {
                const float e = fmaxf(eraw, eps);
                const float R = t > 0 ? matvec(x) : x;
                const float sf = act ? e * fmaxf(R, eps) : 0.f;
                if constexpr (D != 0) gv = mq_sp_gather<D>(sl, sf);
                const float S = mq_sum<D>(sf);
                const float iS = __builtin_amdgcn_rcpf(S);
                const float xn = sf * iS;
                if constexpr (D != 0) { x = sf; vinv = iS; }
                else x = xn;
                lacc += (double)mq_logacc<D>(S);
                if (phase) emit(xn, rbv, t);
                else if (act) o[(size_t)t * q + j] = xn;
            };
            mq_drain();
            int tb = t0;
            for (; tb + MQ_PF <= t1; tb += MQ_PF) {
                float ce[MQ_PF], cr[MQ_PF];
#pragma unroll
                for (int u = 0; u < MQ_PF; ++u) { ce[u] = en[u]; cr[u] = rn[u]; }
                rows.up(tb + MQ_PF, t1, en);
                orows.up(tb + MQ_PF, tr, rn);
#pragma unroll
                for (int u = 0; u < MQ_PF; ++u) step(tb + u, ce[u], cr[u]);
                if (DEC::on && phase && cnt == MQ_RING) drain();
            }
#pragma unroll
            for (int u = 0; u < MQ_PF; ++u)
                if (tb + u < t1) step(tb + u, en[u], rn[u]);            // wave-uniform
            if (!phase) __syncthreads();                    // the backward wave has parked Rb_t for t >= mid
        }
        if (j == 0) ll[row] = lacc * mq_logscale<D>();
    } else {
        float bh = 0.f;
        const MqRows rows(Er, q, j), orows(o, q, j);
        for (int phase = 0; phase < 2; ++phase) {
            const int t0 = phase ? mid - 1 : L - 1, t1 = phase ? 0 : mid;          // t0 down to t1
            const int ta = phase ? t1 : L;                  // phase 0 reads nothing from `out`
            float en[MQ_PF], an[MQ_PF];
            rows.down(t0, t1, en);
            orows.down(t0, ta, an);
            auto step = [&](int t, float eraw, float al) {
                const float e = fmaxf(eraw, eps);
                const float rb = t < L - 1 ? fmaxf(matvec(bh), eps) : 1.f;
                const float sb = act ? e * rb : 0.f;
                if constexpr (D != 0) gv = mq_sp_gather<D>(sl, sb);
                if (phase) emit(al, rb, t);
                else if (act) o[(size_t)t * q + j] = rb;
                const float iS = __builtin_amdgcn_rcpf(mq_sum<D>(sb));
                if constexpr (D != 0) { bh = sb; vinv = iS; }
                else bh = sb * iS;
            };
            mq_drain();
            int tb = t0;
            for (; tb - MQ_PF + 1 >= t1; tb -= MQ_PF) {
                float ce[MQ_PF], ca[MQ_PF];
#pragma unroll
                for (int u = 0; u < MQ_PF; ++u) { ce[u] = en[u]; ca[u] = an[u]; }
                rows.down(tb - MQ_PF, t1, en);
                orows.down(tb - MQ_PF, ta, an);
#pragma unroll
                for (int u = 0; u < MQ_PF; ++u) step(tb - u, ce[u], ca[u]);
                if (DEC::on && phase && cnt == MQ_RING) drain();
            }
#pragma unroll
            for (int u = 0; u < MQ_PF; ++u)
                if (tb - u >= t1) step(tb - u, en[u], an[u]);           // wave-uniform
            if (!phase) __syncthreads();                    // the forward wave has parked alpha_hat_t for t < mid
        }
    }
    drain();
}

template <int QB, int D = 0>
__global__ __launch_bounds__(128) void k_mq_posterior2(const float *__restrict__ A, const float *__restrict__ pi,
                                                       const float *__restrict__ E, int b, int L, int q, float eps,
                                                       float *__restrict__ out, double *__restrict__ ll, int mode,
                                                       const int *__restrict__ need = nullptr,
                                                       const MqSp *__restrict__ sp = nullptr) {
    mq_posterior2_body<QB, D, NoDecode>(A, pi, E, b, L, q, eps, out, ll, mode, need, sp, NoDecode(), nullptr);
}

// k_mq_posterior2 with the DecodeMid output policy; park: the workspace's parking region.
// Dynamic LDS: mq_decode_lds(q) bytes.
template <int QB, int D = 0>
__global__ __launch_bounds__(128) void k_mq_posterior2_decode(const float *__restrict__ A, const float *__restrict__ pi,
                                                              const float *__restrict__ E, int b, int L, int q, float eps,
                                                              float *__restrict__ park, double *__restrict__ ll,
                                                              const int *__restrict__ need, const MqSp *__restrict__ sp,
                                                              const DecodeMid dec) {
    extern __shared__ __attribute__((aligned(16))) float mq_lds[];
    mid_weights(dec, mq_lds);
    mq_posterior2_body<QB, D, DecodeMid>(A, pi, E, b, L, q, eps, park, ll, 0, need, sp, dec, mq_lds);
}
static unsigned mq_decode_lds(int q) { return (unsigned)((MID_WT_FLOATS + 2 * MQ_RING * (q | 1)) * sizeof(float)); }

// sp (or null: dense steps only): room for k MqSp tables, filled here
static void mq_sp_prepare(const float *A, int k, int q, MqSp *sp, hipStream_t st) {
    hipLaunchKernelGGL(k_mq_sp_prep, dim3(k), dim3(64), 0, st, A, sp, q, opt(HMM_OPT_FORCE_DENSE) == 1 ? 1 : 0);
}

static void mq_posterior2(const float *A, const float *pi, const float *E, int k, int b, int L, int q, float eps,
                          float *out, double *ll, int mode, hipStream_t st, const int *need = nullptr, MqSp *sp = nullptr) {
    const dim3 grid((unsigned)(k * b));
    if (sp) {
        mq_sp_prepare(A, k, q, sp, st);
        hipLaunchKernelGGL((k_mq_posterior2<64, 4>), grid, dim3(128), 0, st, A, pi, E, b, L, q, eps, out, ll, mode, need, (const MqSp *)sp);
        hipLaunchKernelGGL((k_mq_posterior2<64, 8>), grid, dim3(128), 0, st, A, pi, E, b, L, q, eps, out, ll, mode, need, (const MqSp *)sp);
    }
    if (q <= 32)
        hipLaunchKernelGGL((k_mq_posterior2<32>), grid, dim3(128), 0, st, A, pi, E, b, L, q, eps, out, ll, mode, need, (const MqSp *)sp);
    else if (q <= 48)
        hipLaunchKernelGGL((k_mq_posterior2<48>), grid, dim3(128), 0, st, A, pi, E, b, L, q, eps, out, ll, mode, need, (const MqSp *)sp);
    else
        hipLaunchKernelGGL((k_mq_posterior2<64>), grid, dim3(128), 0, st, A, pi, E, b, L, q, eps, out, ll, mode, need, (const MqSp *)sp);
}

// the decode form of mq_posterior2 (any L >= 1: at L = 1 the forward wave has the one position and finds Rb = 1
// parked, the arithmetic of mq_forward + mq_backward)
static void mq_posterior2_decode(const float *A, const float *pi, const float *E, int k, int b, int L, int q, float eps,
                                 float *park, double *ll, const DecodeMid &dec, hipStream_t st, const int *need,
                                 MqSp *sp) {
    const dim3 grid((unsigned)(k * b));
    const unsigned lds = mq_decode_lds(q);
    const MqSp *csp = sp;
    if (sp) {
        mq_sp_prepare(A, k, q, sp, st);
        launch(k_mq_posterior2_decode<64, 4>, grid, dim3(128), lds, st, A, pi, E, b, L, q, eps, park, ll, need, csp, dec);
        launch(k_mq_posterior2_decode<64, 8>, grid, dim3(128), lds, st, A, pi, E, b, L, q, eps, park, ll, need, csp, dec);
    }
    auto *kern = q <= 32 ? k_mq_posterior2_decode<32> : q <= 48 ? k_mq_posterior2_decode<48> : k_mq_posterior2_decode<64>;
    launch(kern, grid, dim3(128), lds, st, A, pi, E, b, L, q, eps, park, ll, need, csp, dec);
}

static void mq_forward_signed(const float *A, const float *pi, const float *E, int k, int b, int L, int q, float eps,
                              float *out_alpha, double *ll, hipStream_t st, const int *need = nullptr, MqSp *sp = nullptr) {
    const dim3 grid((unsigned)(k * b));
    float *nos = nullptr;
    const MqSp *csp = sp;
    if (sp) {
        mq_sp_prepare(A, k, q, sp, st);
        hipLaunchKernelGGL((k_mq_forward<64, true, 4>), grid, dim3(64), 0, st, A, pi, E, b, L, q, eps, out_alpha, nos, ll, nos, need, csp);
        hipLaunchKernelGGL((k_mq_forward<64, true, 8>), grid, dim3(64), 0, st, A, pi, E, b, L, q, eps, out_alpha, nos, ll, nos, need, csp);
    }
    if (q <= 32)
        hipLaunchKernelGGL((k_mq_forward<32, true>), grid, dim3(64), 0, st, A, pi, E, b, L, q, eps, out_alpha, nos, ll, nos, need, csp);
    else if (q <= 48)
        hipLaunchKernelGGL((k_mq_forward<48, true>), grid, dim3(64), 0, st, A, pi, E, b, L, q, eps, out_alpha, nos, ll, nos, need, csp);
    else
        hipLaunchKernelGGL((k_mq_forward<64, true>), grid, dim3(64), 0, st, A, pi, E, b, L, q, eps, out_alpha, nos, ll, nos, need, csp);
}

static void mq_forward(const float *A, const float *pi, const float *E, int k, int b, int L, int q, float eps,
                       float *out_alpha, float *log_alpha, double *ll, hipStream_t st, const int *need = nullptr,
                       MqSp *sp = nullptr) {
    const dim3 grid((unsigned)(k * b));
    float *nos = nullptr;
    const MqSp *csp = sp;
    if (sp) {
        mq_sp_prepare(A, k, q, sp, st);
        hipLaunchKernelGGL((k_mq_forward<64, false, 4>), grid, dim3(64), 0, st, A, pi, E, b, L, q, eps, out_alpha, log_alpha, ll, nos, need, csp);
        hipLaunchKernelGGL((k_mq_forward<64, false, 8>), grid, dim3(64), 0, st, A, pi, E, b, L, q, eps, out_alpha, log_alpha, ll, nos, need, csp);
    }
    if (q <= 32)
        hipLaunchKernelGGL((k_mq_forward<32>), grid, dim3(64), 0, st, A, pi, E, b, L, q, eps, out_alpha, log_alpha, ll, nos, need, csp);
    else if (q <= 48)
        hipLaunchKernelGGL((k_mq_forward<48>), grid, dim3(64), 0, st, A, pi, E, b, L, q, eps, out_alpha, log_alpha, ll, nos, need, csp);
    else
        hipLaunchKernelGGL((k_mq_forward<64>), grid, dim3(64), 0, st, A, pi, E, b, L, q, eps, out_alpha, log_alpha, ll, nos, need, csp);
}

static void mq_backward(const float *A, const float *E, int k, int b, int L, int q, float eps, float *out,
                        const double *loglik, int mode, hipStream_t st, const int *need = nullptr, MqSp *sp = nullptr) {
    const dim3 grid((unsigned)(k * b));
    const MqSp *csp = sp;
    if (sp) {
        mq_sp_prepare(A, k, q, sp, st);
        hipLaunchKernelGGL((k_mq_backward<64, 4>), grid, dim3(64), 0, st, A, E, b, L, q, eps, out, loglik, mode, need, csp);
        hipLaunchKernelGGL((k_mq_backward<64, 8>), grid, dim3(64), 0, st, A, E, b, L, q, eps, out, loglik, mode, need, csp);
    }
    if (q <= 32)
        hipLaunchKernelGGL((k_mq_backward<32>), grid, dim3(64), 0, st, A, E, b, L, q, eps, out, loglik, mode, need, csp);
    else if (q <= 48)
        hipLaunchKernelGGL((k_mq_backward<48>), grid, dim3(64), 0, st, A, E, b, L, q, eps, out, loglik, mode, need, csp);
    else
        hipLaunchKernelGGL((k_mq_backward<64>), grid, dim3(64), 0, st, A, E, b, L, q, eps, out, loglik, mode, need, csp);
}

// ------------------------------------------------------------------ gradients of the log-likelihood, 16 < q <= 64
// Same derivatives and clamp handling as hmm_grad.inc (dE = w gamma / E, dA = sum_t xi_t / A,
// dpi = gamma_0 / pi; a clamped predicted state passes nothing back).  dE first holds the signed
// alpha_hat written by k_mq_forward<., true> and is overwritten position by position.  Lane i keeps
// row i of A and row i of G = sum_t alpha_hat_t[i] w / Sg_t * bh_{t+1}[.]: the bh broadcasts of the
// adjoint mat-vec feed both.  gpart[row][i][j] is summed over sequences in a fixed order.
template <int QB>
__global__ __launch_bounds__(64) void k_mq_backward_grad(const float *__restrict__ A, const float *__restrict__ E,
                                                         int b, int L, int q, float eps,
                                                         const float *__restrict__ gw, float *__restrict__ dE,
                                                         float *__restrict__ gpart, const int *__restrict__ need = nullptr) {
    const int row = blockIdx.x, m = row / b, i = threadIdx.x;
    if (need && !need[row]) return;                          // served per chunk (hmm_postgrad_chunked.inc)
    const bool act = i < q;
    const float *Am = A + (size_t)m * q * q;
    float arow[QB], grow[QB];
#pragma unroll
    for (int jj = 0; jj < QB; ++jj) { arow[jj] = (act && jj < q) ? Am[(size_t)i * q + jj] : 0.f; grow[jj] = 0.f; }
    const float *Er = E + (size_t)row * L * q;
    float *o = dE + (size_t)row * L * q;
    const float w = gw ? gw[row] : 1.f;
    float bhm = 0.f;                                        // masked, normalised backward vector of position t + 1
    const MqRows rows(Er, q, i), arows(o, q, i);
    float en[MQ_PF], an[MQ_PF];
    rows.down(L - 1, 0, en);
    arows.down(L - 1, 0, an);
    auto step = [&](int t, float eraw, float als) {
        const float e = fmaxf(eraw, eps);
        const float al = __builtin_fabsf(als);
        const bool live = __builtin_bit_cast(int, als) >= 0;      // predicted state of position t not clamped
        MqDense<QB> bd;                                      // bhm of position t + 1, a row in every row
        float rb = 1.f;
        if (t < L - 1) {
            bd.spread(bhm, i);
            float r4[4] = {0.f, 0.f, 0.f, 0.f};
            MqDenseLoop<QB, 0>::dot(bd, arow, r4);
            rb = fmaxf((r4[0] + r4[1]) + (r4[2] + r4[3]), eps);
        }
        const float g = act ? al * rb : 0.f;
        const float Sg = mq_wave_sum(g);
        const float ig = __builtin_amdgcn_rcpf(Sg);
        // (position 0 keeps w gamma_0 / eps in its clamped entries for k_mq_grad_pi, which zeroes them)
        if (act) o[(size_t)t * q + i] = (eraw > eps || t == 0) ? g * (ig * w) * __builtin_amdgcn_rcpf(e) : 0.f;
        if (t < L - 1) {                                    // transition (t -> t + 1): row i of sum xi / A
            const float coef = act ? al * (ig * w) : 0.f;
            MqDenseLoop<QB, 0>::outer(bd, coef, grow);
        }
        const float sb = act ? e * rb : 0.f;
        const float Sb = mq_wave_sum(sb);
        bhm = live ? sb * __builtin_amdgcn_rcpf(Sb) : 0.f;
    };
    mq_drain();
    int tb = L - 1;
    for (; tb - MQ_PF + 1 >= 0; tb -= MQ_PF) {              // whole blocks: no branch inside
        float ce[MQ_PF], ca[MQ_PF];
#pragma unroll
        for (int u = 0; u < MQ_PF; ++u) { ce[u] = en[u]; ca[u] = an[u]; }
        rows.down(tb - MQ_PF, 0, en);
        arows.down(tb - MQ_PF, 0, an);
#pragma unroll
        for (int u = 0; u < MQ_PF; ++u) step(tb - u, ce[u], ca[u]);
    }
#pragma unroll
    for (int u = 0; u < MQ_PF; ++u)
        if (tb - u >= 0) step(tb - u, en[u], an[u]);        // wave-uniform
    if (act) {
        float *gp = gpart + ((size_t)row * q + i) * q;
#pragma unroll
        for (int jj = 0; jj < QB; ++jj)
            if (jj < q) gp[jj] = grow[jj];
    }
}

// dA[m][e] = sum over the model's b sequences of gpart[row][e], fp64, fixed order: one wave per entry, lane s
// takes sequences s, s + 64, ..., the 64 partials meet in a fixed butterfly
__global__ __launch_bounds__(64) void k_mq_grad_sum(const float *__restrict__ gpart, float *__restrict__ dA, int b, int q) {
    const int m = blockIdx.y, e = blockIdx.x;
    const float *src = gpart + (size_t)m * b * q * q + e;
    double acc = 0.0;
    for (int r = threadIdx.x; r < b; r += 64) acc += (double)src[(size_t)r * q * q];
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if (threadIdx.x == 0) dA[(size_t)m * q * q + e] = (float)acc;
}

// dpi[j] = sum_s dE[s,0,j] * max(E[s,0,j], eps) / pi[j]  (= sum_s w gamma_0 / pi), fixed order.  The sweeps leave
// w gamma_0 / eps in the clamped entries of position 0 (a clamped emission takes the gradient from E, not from pi);
// they are zeroed here.
__global__ __launch_bounds__(64) void k_mq_grad_pi(const float *__restrict__ pi, const float *__restrict__ E,
                                                   float *__restrict__ dE, int b, int L, int q, float eps,
                                                   float *__restrict__ dpi) {
    // one wave per (model, state): lane s takes sequences s, s + 64, ..., fixed butterfly over the 64 partials
    const int m = blockIdx.y, j = blockIdx.x;
    double acc = 0.0;
    for (int s = threadIdx.x; s < b; s += 64) {
        const size_t off = ((size_t)m * b + s) * (size_t)L * q + j;
        const float e = E[off];
        acc += (double)dE[off] * (double)fmaxf(e, eps);
        if (!(e > eps)) dE[off] = 0.f;
    }
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if (threadIdx.x == 0) {
        const float pj = pi[(size_t)m * q + j];
        dpi[(size_t)m * q + j] = pj > eps ? (float)(acc / (double)pj) : 0.f;
    }
}

struct MqGradPlan { size_t o_ll, o_gpart, o_sp, total; };
static void make_mqgradplan(int k, int b, int q, MqGradPlan *p) {
    size_t off = 0;
    p->o_ll = off;    off = align_up(off + (size_t)k * b * sizeof(double));
    p->o_gpart = off; off = align_up(off + (size_t)k * b * q * q * sizeof(float));
    p->o_sp = off;    off = align_up(off + (size_t)k * sizeof(MqSp));     // the forward sweep's sparse-step tables
    p->total = off;
}

// the two sweeps (of the sequences need[] names, or of all) and the sums over sequences: ll (k,b) fp64 and
// gpart (k*b, q, q) in the workspace — rows the caller filled another way are left alone by the sweeps
static int mq_loglik_grad_run(const float *A, const float *pi, const float *E, int k, int b, int L, int q, float eps,
                              const float *gw, float *dA, float *dpi, float *dE, double *loglik, double *ll, float *gpart,
                              hipStream_t st, const int *need = nullptr, MqSp *sp = nullptr);
static int mq_loglik_grad(const float *A, const float *pi, const float *E, int k, int b, int L, int q, float eps,
                          const float *gw, float *dA, float *dpi, float *dE, double *loglik, char *ws, hipStream_t st) {
    MqGradPlan gp;
    make_mqgradplan(k, b, q, &gp);
    return mq_loglik_grad_run(A, pi, E, k, b, L, q, eps, gw, dA, dpi, dE, loglik, (double *)(ws + gp.o_ll),
                              (float *)(ws + gp.o_gpart), st, nullptr, (MqSp *)(ws + gp.o_sp));
}
static int mq_loglik_grad_run(const float *A, const float *pi, const float *E, int k, int b, int L, int q, float eps,
                              const float *gw, float *dA, float *dpi, float *dE, double *loglik, double *ll, float *gpart,
                              hipStream_t st, const int *need, MqSp *sp) {
    mq_forward_signed(A, pi, E, k, b, L, q, eps, dE, ll, st, need, sp);
    const dim3 grid((unsigned)(k * b));
    if (q <= 32)
        hipLaunchKernelGGL((k_mq_backward_grad<32>), grid, dim3(64), 0, st, A, E, b, L, q, eps, gw, dE, gpart, need);
    else if (q <= 48)
        hipLaunchKernelGGL((k_mq_backward_grad<48>), grid, dim3(64), 0, st, A, E, b, L, q, eps, gw, dE, gpart, need);
    else
        hipLaunchKernelGGL((k_mq_backward_grad<64>), grid, dim3(64), 0, st, A, E, b, L, q, eps, gw, dE, gpart, need);
    hipLaunchKernelGGL(k_mq_grad_sum, dim3(q * q, k), dim3(64), 0, st, (const float *)gpart, dA, b, q);
    hipLaunchKernelGGL(k_mq_grad_pi, dim3(q, k), dim3(64), 0, st, pi, E, dE, b, L, q, eps, dpi);
    if (loglik)
        hipLaunchKernelGGL(k_copy_loglik, dim3((k * b + 255) / 256), dim3(256), 0, st, (const double *)ll, loglik, k * b);
    return check_launch();
}
