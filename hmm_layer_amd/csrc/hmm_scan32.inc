// hmm_scan32.inc — the chunked (time-parallel) scan for 17..32 states, included by hmm_engine.hip.
//
// The 29-state two-copy gene model (hmm_layer/gene_pred_hmm_transitioner.py:263-308,
// GenePredMultiHMMTransitioner(k = 2)) does not fit the 16-state MFMA tile of the main pipeline and
// ran, in round 1, one dependent chain per sequence (hmm_midq.inc: 72 ms for b = 1024 x L = 1e5 against
// 7 ms for 15 states).  Here it gets the same three phases with 32-state tiles:
//
//   reduce   k_reduce_sparse_wide<TopoGene29>: the sparse-topology reduce of the main pipeline, 32 lanes per
//            chain (one operator column per lane, 45 structural fma's), two chains per wave
//   scan     k32_scan: chunk-level prefix / suffix hops over 32 x 32 operators, one wave per direction
//   apply    k32_forward / k32_backward: the apply kernels with TWO 16-state MFMA tiles per chain
//            (a 32-state vector is two tile rows; a step is four 16x16x16 block products), exact
//            cell step semantics, alpha_hat checkpoints every 4 steps, posteriors staged in LDS
//
// Which models take this path is decided on the device (k32_check): the support of A must lie inside the
// compiled topology and be primitive (see k_topo_check); everything else — other 17..32-state
// models, and sequences whose certificate (psi, or the one-directional CERT / CERT3 sums) fires or that a reduce
// marked (k32_select) — is served by the
// one-wave-per-sequence kernels of hmm_midq.inc, which implement the cell's serial semantics exactly and
// take a per-sequence mask.  hmm_posterior (all modes), hmm_forward and hmm_backward use this path; the
// gradients run per chunk of this plan for up to 512 sequences (hmm_postgrad_chunked.inc), otherwise — and Viterbi
// always — on hmm_midq.inc.  This file holds the kernels; the plan (MidPlan) and the host drivers (scan_*<Scan32>)
// are shared with the 64-state rows: hmm_scan_mid.inc.

#define Q32 32
#define SUB32 4                       // steps per apply block = checkpoint spacing
#define OUT32_ROWS 8                  // rows per chain staged in LDS per flush
#define OUT32_STRIDE (OUT32_ROWS * Q32 + 4)
#define OUT32_SEG (16 * OUT32_STRIDE + 32)

// elig[m]: 0 = the serial kernels serve this model (support not primitive, or the routing is forced);
// TopoGene29::ID (| TOPO_UNIT) = the chunked scan with the compiled sparse reduce; ID_DENSE32 = the chunked scan
// with the dense MFMA reduce (any other primitive model of 17..32 states: a learned dense A, other topologies).
// One wave per model.
#define ID_DENSE32 4
#define ID_DENSE64 5                  // (hmm_scan64.inc's k64_check; k32_select serves both plans)
__global__ __launch_bounds__(64) void k32_check(const float *__restrict__ A, int *__restrict__ elig, int q,
                                                int exact_mode, float eps, int *__restrict__ nex,
                                                int opt_force_dense32 = 0) {
    typedef TopoGene29 T;
    const int m = blockIdx.x, lane = threadIdx.x;
    const float *Am = A + (size_t)m * q * q;
    if (m == 0 && lane == 0) *nex = 0;
    const bool forced = exact_mode == HMM_EXACT_ALWAYS || exact_mode == HMM_EXACT_ALWAYS_NARROW;
    bool out29 = q != T::Q || opt_force_dense32;
    bool nonunit = false;                  // an edge out of a single-successor state that is not exactly 1
    if (!out29)
        for (int e = lane; e < q * q; e += 64) {
            const float a = Am[e];
            const int i = e / q, j = e - i * q;
            const bool in = edge_in<T>(i, j);
            out29 = out29 || (a != 0.f && !in);
            nonunit = nonunit || (in && a != 1.0f && out_degree<T>(i) == 1);
        }
    out29 = __ballot(out29) != 0ull;
    nonunit = __ballot(nonunit) != 0ull;
    bool bad = forced;
    if (!bad && exact_mode == HMM_EXACT_AUTO) {
        // primitive support: B^1024 > 0 (Wielandt: (q-1)^2 + 1 = 962 suffices for q = 32)
        unsigned row = 0;
        if (lane < q)
            for (int j = 0; j < q; ++j) row |= (Am[lane * q + j] > eps) ? (1u << j) : 0u;
        for (int it = 0; it < 10; ++it) {
            unsigned nr = 0;
            for (int j = 0; j < q; ++j) {
                const unsigned rj = (unsigned)__builtin_amdgcn_readlane((int)row, j);
                nr |= ((row >> j) & 1u) ? rj : 0u;
            }
            row = nr;
        }
        const unsigned full = q >= 32 ? 0xffffffffu : ((1u << q) - 1u);
        bad = __ballot(lane < q && row != full) != 0ull;
    }
    if (lane == 0) elig[m] = bad ? 0 : (out29 ? ID_DENSE32 : (T::ID | (nonunit ? 0 : TOPO_UNIT)));
}

// ---- scan over 32 x 32 chunk operators: ops[chain][i][k] (i = state at the chunk's last step, k = state
// just before the chunk, column k scaled by 2^-exps[k]).  One 128-thread block per sequence, wave 0 the
// forward prefix chain, wave 1 the backward suffix chain; lanes 0..31 carry the vector, lanes 32..63 zeros
// (all lanes stay active: the wave-wide sums and maxima are DPP / permlane reductions).
__device__ __forceinline__ float wave_sum32(float v) { return col_sum(row_sum_f(v)); }
__device__ __forceinline__ int wave_max32(int v) { return col_max_i(row_max_i(v)); }

__global__ __launch_bounds__(128) void k32_scan(const float *__restrict__ pi, const float *__restrict__ ops,
                                               const int *__restrict__ exps, float *__restrict__ prefix,
                                               double *__restrict__ llpre, float *__restrict__ suffix,
                                               double *__restrict__ lsuf, double *__restrict__ loglik,
                                               const int *__restrict__ elig, Plan p, float eps) {
    const int seq = blockIdx.x;
    const int lane = threadIdx.x & 63;
    const int dir = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int q = p.q, C = p.C;
    const int m = seq / p.b;
    if (elig[m] == 0) return;
    const size_t chain0 = (size_t)seq * C;
    const bool act = lane < q;
    const int n = lane & 31;
    if (dir == 0) {
        const float praw = act ? pi[(size_t)m * q + lane] : 0.f;
        float a = act ? fmaxf(praw, eps) : 0.f;
        double ll = 0.0;
        if (lane < Q32) prefix[chain0 * Q32 + lane] = praw;
        if (lane == 0) llpre[chain0] = 0.0;
        f4 rw[8];                                            // row n of the next operator, one hop ahead
        int xe = 0;
        auto fetch = [&](int c) {
            const f4 *row = reinterpret_cast<const f4 *>(ops + (chain0 + c) * Q32 * Q32 + n * Q32);
#pragma unroll
            for (int u = 0; u < 8; ++u) rw[u] = row[u];
            xe = exps[(chain0 + c) * Q32 + n];
        };
        fetch(0);
        for (int c = 0; c < C; ++c) {
            f4 cur[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) cur[u] = rw[u];
            const int xec = xe;
            if (c + 1 < C) fetch(c + 1);
            const int we = (a > 0.f) ? __builtin_amdgcn_frexp_expf(a) + xec : -(1 << 28);
            const int emax = wave_max32(we);
            int sh = xec - emax;
            sh = sh < -300 ? -300 : sh;
            const float w = __builtin_amdgcn_ldexpf(a, sh);
            float acc = 0.f;
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                acc = fmaf(cur[u].x, lane_bcast(w, 4 * u + 0), acc);
                acc = fmaf(cur[u].y, lane_bcast(w, 4 * u + 1), acc);
                acc = fmaf(cur[u].z, lane_bcast(w, 4 * u + 2), acc);
                acc = fmaf(cur[u].w, lane_bcast(w, 4 * u + 3), acc);
            }
            acc = act ? acc : 0.f;
            const float S = wave_sum32(acc);
            a = acc / S;
            ll += (double)__logf(S) + (double)emax * LN2;
            if (c + 1 < C) {
                if (lane < Q32) prefix[(chain0 + c + 1) * Q32 + lane] = a;
                if (lane == 0) llpre[chain0 + c + 1] = ll;
            }
        }
        if (lane == 0) loglik[seq] = ll;
    } else {
        float v = act ? 1.f : 0.f;
        double lb = 0.0;
        float col[Q32];                                      // column n of the next operator
        int xe = 0;
        auto fetch = [&](int c) {
            const float *X = ops + (chain0 + c) * Q32 * Q32;
#pragma unroll
            for (int j = 0; j < Q32; ++j) col[j] = X[j * Q32 + n];
            xe = exps[(chain0 + c) * Q32 + n];
        };
        if (C > 1) fetch(C - 1);
        for (int c = C - 1; c >= 0; --c) {
            if (lane < Q32) suffix[(chain0 + c) * Q32 + lane] = v;
            if (lane == 0) lsuf[chain0 + c] = lb;
            if (c == 0) break;
            float cc[Q32];
#pragma unroll
            for (int j = 0; j < Q32; ++j) cc[j] = col[j];
            const int xec = xe;
            if (c - 1 > 0) fetch(c - 1);
            float u = 0.f;
#pragma unroll
            for (int j = 0; j < Q32; ++j) u = fmaf(cc[j], lane_bcast(v, j), u);
            u = act ? u : 0.f;
            const int we = (u > 0.f) ? __builtin_amdgcn_frexp_expf(u) + xec : -(1 << 28);
            const int emax = wave_max32(we);
            int sh = xec - emax;
            sh = sh < -300 ? -300 : sh;
            v = __builtin_amdgcn_ldexpf(u, sh);
            lb += (double)emax * LN2;
        }
    }
}

// ---- apply kernels, two 16-state tiles per chain.  Lane (g, n) holds states 16 t + 4g .. + 3 of chain n in
// X[t], t = 0, 1.  A step's mat-vec is four 16x16x16 block products: D[r] = sum_c Aop[r][c] * X[c].
struct A32 { float f[2][2][4], b[2][2][4]; };       // forward (A^T) and backward (A) MFMA A-operands per block

__device__ __forceinline__ void load_A32(const float *A, int q, int g, int n, A32 &a) {
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                const int s = 16 * c + 4 * g + kk, d = 16 * r + n;       // contraction index, output row
                const bool ok = s < q && d < q;
                a.f[r][c][kk] = ok ? A[s * q + d] : 0.f;                  // alpha' = A^T alpha
                a.b[r][c][kk] = ok ? A[d * q + s] : 0.f;                  // R = A bh
            }
}

struct X32 { f4 t[2]; };

__device__ __forceinline__ X32 matvec32(const float (&aop)[2][2][4], const X32 &x) {
    X32 d;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const f4 z = {0.f, 0.f, 0.f, 0.f};
        d.t[r] = mfma4v((f4){aop[r][0][0], aop[r][0][1], aop[r][0][2], aop[r][0][3]}, x.t[0], z);
        d.t[r] = mfma4v((f4){aop[r][1][0], aop[r][1][1], aop[r][1][2], aop[r][1][3]}, x.t[1], d.t[r]);
    }
    return d;
}
__device__ __forceinline__ float sum32(const X32 &x) { return col_sum(hsum(x.t[0]) + hsum(x.t[1])); }

struct B32 { Bounds t[2]; };
__device__ __forceinline__ B32 make_bounds32(int g, int q, float eps) {
    B32 b;
    const float inf = __builtin_inff();
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int s0 = 16 * t + 4 * g;
        b.t[t].lo.x = s0 + 0 < q ? eps : 0.f;  b.t[t].hi.x = s0 + 0 < q ? inf : 0.f;
        b.t[t].lo.y = s0 + 1 < q ? eps : 0.f;  b.t[t].hi.y = s0 + 1 < q ? inf : 0.f;
        b.t[t].lo.z = s0 + 2 < q ? eps : 0.f;  b.t[t].hi.z = s0 + 2 < q ? inf : 0.f;
        b.t[t].lo.w = s0 + 3 < q ? eps : 0.f;  b.t[t].hi.w = s0 + 3 < q ? inf : 0.f;
    }
    return b;
}

// emission rows s = 0 .. N-1 of this lane's chain: two 16-byte loads per row (states 4g.. and 16+4g..);
// what lies past the row's q states is the next row (or, at the tensor's end, outside the descriptor: 0)
// and is zeroed by the clamp bounds
template <int N>
__device__ __forceinline__ void ld_rows32(__amdgpu_buffer_rsrc_t r, int voff, int rowb, X32 (&e)[N]) {
#pragma unroll
    for (int s = 0; s < N; ++s) {
        e[s].t[0] = __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(r, voff + s * rowb, 0, 0));
        e[s].t[1] = __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(r, voff + s * rowb + 64, 0, 0));
    }
}
__device__ __forceinline__ X32 clamp32(const X32 &e, const B32 &b) {
    X32 r;
    r.t[0] = clampE(e.t[0], b.t[0]);
    r.t[1] = clampE(e.t[1], b.t[1]);
    return r;
}

// one exact forward cell step: X <- normalise(max(E,eps) * max(X A, eps)); *logS = log of the normaliser
__device__ __forceinline__ X32 fwd_step32(const A32 &a, const X32 &x, const X32 &e, bool init, float eps, float *logS) {
    const X32 d = matvec32(a.f, x);
    X32 sf;
#pragma unroll
    for (int t = 0; t < 2; ++t) sf.t[t] = fmax4(sel4(init, x.t[t], d.t[t]), eps) * e.t[t];
    const float S = sum32(sf);
    const float inv = __builtin_amdgcn_rcpf(S);
    *logS = __logf(S);
    sf.t[0] = sf.t[0] * inv;
    sf.t[1] = sf.t[1] * inv;
    return sf;
}

struct Tile32 {
    long long wave, chain;
    bool valid, first;
    int len, voff, m;
    __amdgpu_buffer_rsrc_t rsE;
    const float *baseE;
};

__device__ __forceinline__ Tile32 make_tile32(const float *E, const Plan &p, long long wave, int g, int n) {
    const long long per_model = (long long)p.b * p.C;
    const long long wpm = (per_model + 15) / 16;
    Tile32 tl;
    tl.wave = wave;
    tl.m = (int)(wave / wpm);
    const long long w = wave - (long long)tl.m * wpm;
    const long long c0 = (long long)tl.m * per_model + w * 16;
    tl.valid = w * 16 + n < per_model;
    tl.chain = c0 + (tl.valid ? n : 0);
    const long long seq = tl.chain / p.C;
    const int c = (int)(tl.chain - seq * p.C);
    const long long seq0 = c0 / p.C;
    const int cc0 = (int)(c0 - seq0 * p.C);
    tl.first = c == 0;
    tl.len = tl.valid ? min(p.T, p.L - c * p.T) : 0;
    const long long row0 = seq0 * p.L + (long long)cc0 * p.T;
    const long long row = seq * p.L + (long long)c * p.T;
    tl.voff = (int)((row - row0) * p.q * (long long)sizeof(float)) + g * 16;
    const unsigned long long total = (unsigned long long)p.NB * p.L * p.q * sizeof(float);
    tl.baseE = E + row0 * p.q;
    tl.rsE = make_rsrc(tl.baseE, total - (unsigned long long)row0 * p.q * sizeof(float));
    return tl;
}

// output rows staged in wave-private LDS (per chain one contiguous run of rows, its image in HBM) and
// flushed as 16-byte pieces of contiguous memory — the OutStage of the 16-state kernels for rows of up to
// 32 states
struct Out32 {
    float *seg;                 // 16 chains x OUT32_STRIDE floats, then the chain table [voff x 16][len x 16]
    char *base;
    int q;
};
__device__ __forceinline__ Out32 make_out32(float *seg, char *base, int q, int lane, int voff0, int len) {
    Out32 o = {seg, base, q};
    int *tab = reinterpret_cast<int *>(seg + 16 * OUT32_STRIDE);
    if (lane < 16) { tab[lane] = voff0; tab[16 + lane] = len; }
    __builtin_amdgcn_wave_barrier();
    return o;
}
__device__ __forceinline__ void stage32(const Out32 &o, int n, int g, int srow, const X32 &v) {
    float *pr = o.seg + n * OUT32_STRIDE + srow * o.q;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int s0 = 16 * t + 4 * g;
        if (s0 + 0 < o.q) pr[s0 + 0] = v.t[t].x;
        if (s0 + 1 < o.q) pr[s0 + 1] = v.t[t].y;
        if (s0 + 2 < o.q) pr[s0 + 2] = v.t[t].z;
        if (s0 + 3 < o.q) pr[s0 + 3] = v.t[t].w;
    }
}
__device__ __forceinline__ void flush32(const Out32 &o, int lane, int row0, int nrows) {
    const int *tab = reinterpret_cast<const int *>(o.seg + 16 * OUT32_STRIDE);
    const int ppc = nrows * o.q / 4;
    const float inv = 1.0f / (float)ppc;
    __builtin_amdgcn_wave_barrier();
    for (int pc = lane; pc < 16 * ppc; pc += 64) {
        const int c = (int)(((float)pc + 0.5f) * inv);
        const int kk = pc - c * ppc;
        int rows = tab[16 + c] - row0;
        rows = rows > nrows ? nrows : rows;
        const int nfl = rows * o.q - 4 * kk;
        if (nfl <= 0) continue;
        const f4 v = *reinterpret_cast<const f4 *>(o.seg + c * OUT32_STRIDE + 4 * kk);
        char *dst = o.base + tab[c] + (row0 * o.q + 4 * kk) * (int)sizeof(float);
#if HMM_NT_STORE
        if (nfl >= 4) { __builtin_nontemporal_store(v, reinterpret_cast<f4u *>(dst)); }
#else
        if (nfl >= 4) { P4 t = {v.x, v.y, v.z, v.w}; *reinterpret_cast<P4 *>(dst) = t; }
#endif
        else if (nfl == 3) { P3 t = {v.x, v.y, v.z}; *reinterpret_cast<P3 *>(dst) = t; }
        else if (nfl == 2) { P2 t = {v.x, v.y}; *reinterpret_cast<P2 *>(dst) = t; }
        else { *reinterpret_cast<float *>(dst) = v.x; }
    }
    __builtin_amdgcn_wave_barrier();
}

// max(d, eps)'s clamp-born part, component-wise: where the clamp was active the whole eps is born there, elsewhere the
// carried clamp-born part df (forward_body's CERT / backward_body's CERT3 in hmm_engine.hip)
__device__ __forceinline__ f4 born4(f4 d, f4 df, float eps) {
    f4 r = {d.x > eps ? df.x : eps, d.y > eps ? df.y : eps, d.z > eps ? df.z : eps, d.w > eps ? df.w : eps};
    return r;
}
__device__ __forceinline__ float dot32(const X32 &a, const X32 &b) {
    return col_sum(hsum(a.t[0] * b.t[0]) + hsum(a.t[1] * b.t[1]));
}

// LOGA = false, CERT = false: alpha_hat entering every SUB32-step block -> ckpt ([wave][block][chain][32]), nothing else;
// LOGA = true: log alpha_t = log alpha_hat_t + sum_{s<=t} log c_s -> out (hmm_forward with log alpha)
// CERT (hmm_forward, which has no backward pass to sum psi in): forward_body's CERT in hmm_engine.hip — the part of
//   alpha_hat born from the forward cell's clamps inside this chunk is carried along (Fv) and weighed at the chunk's
//   last position with the chunk scan's suffix vector there -> phi[chain]; with LOGA also the clamp-born share of
//   alpha_hat itself at the chunk's end, and what it becomes under the next observation (shnext).  CERT without LOGA
//   (the log-likelihood alone) writes nothing but phi.
template <bool LOGA, bool CERT = false>
__global__ __launch_bounds__(256) void k32_forward(const float *__restrict__ A, const float *__restrict__ E,
                                                   const float *__restrict__ prefix, const double *__restrict__ llpre,
                                                   float *__restrict__ ckpt, float *__restrict__ out,
                                                   const int *__restrict__ elig, Plan p, float eps, long long nwaves,
                                                   const float *__restrict__ suffix = nullptr, float *__restrict__ phi = nullptr) {
    constexpr bool CKPT = !LOGA && !CERT;
    const long long wave = (long long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (wave >= nwaves) return;
    const int lane = threadIdx.x & 63, g = lane >> 4, n = lane & 15;
    const int q = p.q;
    const Tile32 tl = make_tile32(E, p, wave, g, n);
    if (elig[tl.m] == 0) return;
    A32 a;
    load_A32(A + (size_t)tl.m * q * q, q, g, n, a);
    const B32 bd = make_bounds32(g, q, eps);
    const int rowb = q * (int)sizeof(float);
    X32 X;
    X.t[0] = *reinterpret_cast<const f4 *>(prefix + (size_t)tl.chain * Q32 + 4 * g);
    X.t[1] = *reinterpret_cast<const f4 *>(prefix + (size_t)tl.chain * Q32 + 16 + 4 * g);
    const f4 zero4 = {0.f, 0.f, 0.f, 0.f};
    X32 Fv, Xc = X, Fc;                                      // CERT: clamp-born part of X; both at the chain's last step
    Fv.t[0] = Fv.t[1] = Fc.t[0] = Fc.t[1] = zero4;
    float *ck = CKPT ? ckpt + (((size_t)wave * p.nsub) * 16 + n) * Q32 + 4 * g : nullptr;
    __shared__ __attribute__((aligned(16))) float ostage[LOGA ? 4 * OUT32_SEG : 4];
    Out32 os = {};
    if (LOGA)
        os = make_out32(ostage + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) * OUT32_SEG,
                        reinterpret_cast<char *>(out + (tl.baseE - E)), q, lane, tl.voff - g * 16, tl.len);
    double llb = LOGA ? llpre[tl.chain] : 0.0;
    constexpr int GB = OUT32_ROWS / SUB32;
    int voff = tl.voff;
    X32 en[SUB32];
    ld_rows32<SUB32>(tl.rsE, voff, rowb, en);
    for (int j = 0; j < p.nsub; ++j) {
        if (CKPT && tl.valid && j * SUB32 < tl.len) {
            *reinterpret_cast<f4 *>(ck + (size_t)j * 16 * Q32) = X.t[0];
            *reinterpret_cast<f4 *>(ck + (size_t)j * 16 * Q32 + 16) = X.t[1];
        }
        X32 e[SUB32];
#pragma unroll
        for (int s = 0; s < SUB32; ++s) e[s] = en[s];
        if (j + 1 < p.nsub) ld_rows32<SUB32>(tl.rsE, voff + SUB32 * rowb, rowb, en);
        float lacc = 0.f;
#pragma unroll
        for (int s = 0; s < SUB32; ++s) {
            const bool init = tl.first && j == 0 && s == 0;
            float lS;
            if (CERT) {
                const X32 ec = clamp32(e[s], bd);
                const X32 d = matvec32(a.f, X), df = matvec32(a.f, Fv);
                X32 sf, rb;
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    sf.t[t] = fmax4(sel4(init, X.t[t], d.t[t]), eps) * ec.t[t];
                    rb.t[t] = sel4(init, Fv.t[t], born4(d.t[t], df.t[t], eps)) * ec.t[t];   // (pi's own clamp: the scan has it)
                }
                const float S = sum32(sf);
                const float inv = __builtin_amdgcn_rcpf(S);
                lS = __logf(S);
                const bool last = j * SUB32 + s + 1 == tl.len;
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    X.t[t] = sf.t[t] * inv;
                    Fv.t[t] = rb.t[t] * inv;
                    Xc.t[t] = sel4(last, X.t[t], Xc.t[t]);
                    Fc.t[t] = sel4(last, Fv.t[t], Fc.t[t]);
                }
            } else {
                X = fwd_step32(a, X, clamp32(e[s], bd), init, eps, &lS);
            }
            if (LOGA) {
                lacc += (j * SUB32 + s < tl.len) ? lS : 0.f;
                const float base = (float)(llb + (double)lacc);
                X32 la;
                la.t[0] = log4(X.t[0]) + base;
                la.t[1] = log4(X.t[1]) + base;
                stage32(os, n, g, (j % GB) * SUB32 + s, la);
            }
        }
        if (LOGA) {
            llb += (double)lacc;
            if ((j + 1) % GB == 0 || j + 1 == p.nsub) flush32(os, lane, (j / GB) * OUT32_ROWS, (j % GB + 1) * SUB32);
        }
        voff += SUB32 * rowb;
    }
    if (CERT) {
        X32 sv;
        sv.t[0] = *reinterpret_cast<const f4 *>(suffix + (size_t)tl.chain * Q32 + 4 * g);
        sv.t[1] = *reinterpret_cast<const f4 *>(suffix + (size_t)tl.chain * Q32 + 16 + 4 * g);
        float c = dot32(Fc, sv) * __builtin_amdgcn_rcpf(dot32(Xc, sv));
        if (LOGA) {
            // the clamp-born share of alpha_hat where the chunk hands over, and what it becomes one step on under the
            // next observation (the first row of the chunk after, whose kernel starts from the floor-free prefix vector)
            X32 en1;
            en1.t[0] = en1.t[1] = zero4;
            const bool more = tl.valid && tl.chain % p.C != p.C - 1;            // (not the sequence's last chunk)
            if (more) {
                X32 r1[1];
                ld_rows32<1>(tl.rsE, tl.voff + tl.len * rowb, rowb, r1);
                en1 = clamp32(r1[0], bd);
            }
            X32 dx = matvec32(a.f, Xc);
            const X32 df = matvec32(a.f, Fc);
            dx.t[0] = fmax4(dx.t[0], eps);
            dx.t[1] = fmax4(dx.t[1], eps);
            const float dn = dot32(en1, dx);
            const float shnext = (more && dn > 0.f) ? dot32(en1, df) * __builtin_amdgcn_rcpf(dn) : 0.f;
            c = fmaxf(fmaxf(c, sum32(Fc)), shnext);
        }
        if (tl.valid && g == 0) phi[tl.chain] = c;
    }
}

// posteriors.  MODE 0: gamma, 1: log gamma, 2: log gamma + loglik, 3: log beta (no forward part).
// phi: psi, the posterior mass of clamp-born paths (backward_body in hmm_engine.hip), per chain.
// CERT3 (MODE 3, hmm_backward): backward_body's CERT3 — the part of R born from the reverse cell's clamps inside this
//   chunk is carried along (Gv) and weighed at the chunk's first position with alpha_hat there, one forward step from
//   the chunk scan's prefix vector (a uniform start); also the clamp-born share of R where the chunk hands over to the
//   one before, and what it becomes under that chunk's last observation -> phi[chain]
template <int MODE, bool CERT3 = false>
__global__ __launch_bounds__(256) void k32_backward(const float *__restrict__ A, const float *__restrict__ E,
                                                    const float *__restrict__ ckpt, const float *__restrict__ suffix,
                                                    const double *__restrict__ lsuf, const double *__restrict__ loglik,
                                                    float *__restrict__ out, float *__restrict__ phi,
                                                    const int *__restrict__ elig, Plan p, float eps, long long nwaves,
                                                    const float *__restrict__ prefix = nullptr) {
    static_assert(!CERT3 || MODE == 3, "CERT3 is the log beta certificate");
    const long long wave = (long long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (wave >= nwaves) return;
    const int lane = threadIdx.x & 63, g = lane >> 4, n = lane & 15;
    const int q = p.q;
    const Tile32 tl = make_tile32(E, p, wave, g, n);
    if (elig[tl.m] == 0) return;
    A32 a;
    load_A32(A + (size_t)tl.m * q * q, q, g, n, a);
    const B32 bd = make_bounds32(g, q, eps);
    const int rowb = q * (int)sizeof(float);
    __shared__ __attribute__((aligned(16))) float ostage[4 * OUT32_SEG];
    float *seg = ostage + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) * OUT32_SEG;
    const Out32 os = make_out32(seg, reinterpret_cast<char *>(out + (tl.baseE - E)), q, lane, tl.voff - g * 16, tl.len);

    X32 Rv;
    Rv.t[0] = *reinterpret_cast<const f4 *>(suffix + (size_t)tl.chain * Q32 + 4 * g);
    Rv.t[1] = *reinterpret_cast<const f4 *>(suffix + (size_t)tl.chain * Q32 + 16 + 4 * g);
    float llf = 0.f;
    if (MODE == 2) llf = (float)loglik[tl.chain / p.C];
    double lbb = MODE == 3 ? lsuf[tl.chain] : 0.0;
    const float *ck = MODE == 3 ? nullptr : ckpt + (((size_t)wave * p.nsub) * 16 + n) * Q32 + 4 * g;
    float phiacc = 0.f;
    const f4 zero4 = {0.f, 0.f, 0.f, 0.f};
    X32 Gv, Rc = Rv, Gc, ec0;                                // CERT3: clamp-born part of R; R, Gv, E at the first position
    Gv.t[0] = Gv.t[1] = Gc.t[0] = Gc.t[1] = ec0.t[0] = ec0.t[1] = zero4;

    X32 en[SUB32];
    ld_rows32<SUB32>(tl.rsE, tl.voff + (p.nsub - 1) * SUB32 * rowb, rowb, en);
    X32 Xn;
    Xn.t[0] = Xn.t[1] = zero4;
    if (MODE != 3 && tl.valid && (p.nsub - 1) * SUB32 < tl.len) {
        Xn.t[0] = *reinterpret_cast<const f4 *>(ck + (size_t)(p.nsub - 1) * 16 * Q32);
        Xn.t[1] = *reinterpret_cast<const f4 *>(ck + (size_t)(p.nsub - 1) * 16 * Q32 + 16);
    }
    constexpr int GB = OUT32_ROWS / SUB32;                  // blocks per flush group
    for (int j = p.nsub - 1; j >= 0; --j) {
        const int srow = (j % GB) * SUB32;
        X32 e[SUB32];
#pragma unroll
        for (int s = 0; s < SUB32; ++s) e[s] = clamp32(en[s], bd);
        const X32 Xc = Xn;
        if (j > 0) {
            ld_rows32<SUB32>(tl.rsE, tl.voff + (j - 1) * SUB32 * rowb, rowb, en);
            if (MODE != 3 && tl.valid && (j - 1) * SUB32 < tl.len) {
                Xn.t[0] = *reinterpret_cast<const f4 *>(ck + (size_t)(j - 1) * 16 * Q32);
                Xn.t[1] = *reinterpret_cast<const f4 *>(ck + (size_t)(j - 1) * 16 * Q32 + 16);
            }
        }
        // (alpha_hat and R carry "the clamp of this component's prediction was active" in their sign bits: psi,
        // see backward_body in hmm_engine.hip)
        X32 fa[SUB32];
        if (MODE != 3) {
            X32 X = Xc;
#pragma unroll
            for (int s = 0; s < SUB32; ++s) {
                const bool init = tl.first && j == 0 && s == 0;
                const X32 d = matvec32(a.f, X);
                X32 sf;
#pragma unroll
                for (int t = 0; t < 2; ++t)
                    sf.t[t] = sel4(init, fmax4(X.t[t], eps), clamp_flag4(d.t[t], eps)) * e[s].t[t];
                const float inv = __builtin_amdgcn_rcpf(col_sum(hsum_abs(sf.t[0]) + hsum_abs(sf.t[1])));
                fa[s].t[0] = sf.t[0] * inv;
                fa[s].t[1] = sf.t[1] * inv;
                X.t[0] = abs4(fa[s].t[0]);
                X.t[1] = abs4(fa[s].t[1]);
            }
        }
        float lacc = 0.f;
#pragma unroll
        for (int s = SUB32 - 1; s >= 0; --s) {
            const bool act = j * SUB32 + s < tl.len;
            X32 gm;
            if (MODE == 3) {
                const float base = (float)(lbb + (double)lacc);
                gm.t[0] = log4(Rv.t[0]) + base;
                gm.t[1] = log4(Rv.t[1]) + base;
            } else {
                gm.t[0] = fa[s].t[0] * Rv.t[0];         // negative where exactly one of the two clamps was active
                gm.t[1] = fa[s].t[1] * Rv.t[1];
                const float Sg = col_sum(hsum_abs(gm.t[0]) + hsum_abs(gm.t[1]));
                const float ig = __builtin_amdgcn_rcpf(Sg);
                phiacc = fmaf(hsum_neg(gm.t[0]) + hsum_neg(gm.t[1]), act ? ig : 0.f, phiacc);
                if (MODE == 0) {
                    gm.t[0] = mul_abs4(gm.t[0], f4{ig, ig, ig, ig});
                    gm.t[1] = mul_abs4(gm.t[1], f4{ig, ig, ig, ig});
                } else {
                    const float lg = __logf(Sg) - llf;
                    gm.t[0] = log4(abs4(gm.t[0])) - lg;
                    gm.t[1] = log4(abs4(gm.t[1])) - lg;
                }
            }
            stage32(os, n, g, srow + s, gm);
            if (CERT3 && s == 0) { Rc = Rv; Gc = Gv; ec0 = e[0]; }      // (the last block executed is the chunk's first)
            X32 sf;
            sf.t[0] = MODE == 3 ? e[s].t[0] * Rv.t[0] : mul_abs4(Rv.t[0], e[s].t[0]);
            sf.t[1] = MODE == 3 ? e[s].t[1] * Rv.t[1] : mul_abs4(Rv.t[1], e[s].t[1]);
            const float Sb = sum32(sf);
            if (MODE == 3) lacc += act ? __logf(Sb) : 0.f;
            const float ib = __builtin_amdgcn_rcpf(Sb);
            sf.t[0] = sf.t[0] * ib;
            sf.t[1] = sf.t[1] * ib;
            const X32 d = matvec32(a.b, sf);
            if (CERT3) {
                X32 gs;
                gs.t[0] = e[s].t[0] * Gv.t[0] * ib;
                gs.t[1] = e[s].t[1] * Gv.t[1] * ib;
                const X32 ug = matvec32(a.b, gs);
                Gv.t[0] = sel4(act, born4(d.t[0], ug.t[0], eps), Gv.t[0]);
                Gv.t[1] = sel4(act, born4(d.t[1], ug.t[1], eps), Gv.t[1]);
            }
            Rv.t[0] = sel4(act, MODE == 3 ? fmax4(d.t[0], eps) : clamp_flag4(d.t[0], eps), Rv.t[0]);
            Rv.t[1] = sel4(act, MODE == 3 ? fmax4(d.t[1], eps) : clamp_flag4(d.t[1], eps), Rv.t[1]);
        }
        if (MODE == 3) lbb += (double)lacc;
        if (j % GB == 0) {
            const int top = p.nsub - j;
            flush32(os, lane, j * SUB32, (top < GB ? top : GB) * SUB32);
        }
    }
    phiacc = col_sum(phiacc);
    if (MODE != 3 && g == 0 && tl.valid) phi[tl.chain] = phiacc;
    if (CERT3) {
        // alpha_hat at the chunk's first position, up to scale: one forward step from the vector entering the chunk
        X32 P, a0;
        P.t[0] = *reinterpret_cast<const f4 *>(prefix + (size_t)tl.chain * Q32 + 4 * g);
        P.t[1] = *reinterpret_cast<const f4 *>(prefix + (size_t)tl.chain * Q32 + 16 + 4 * g);
        const X32 dp = matvec32(a.f, P);
        a0.t[0] = fmax4(sel4(tl.first, P.t[0], dp.t[0]), eps) * ec0.t[0];
        a0.t[1] = fmax4(sel4(tl.first, P.t[1], dp.t[1]), eps) * ec0.t[1];
        float c = dot32(a0, Gc) * __builtin_amdgcn_rcpf(dot32(a0, Rc));
        c = fmaxf(c, sum32(Gv) * __builtin_amdgcn_rcpf(sum32(Rv)));        // what the chunk before does not get
        // ... and what that share becomes under the last row of the chunk before (whose kernel starts from the chunk
        // scan's floor-free suffix vector)
        X32 ep;
        ep.t[0] = ep.t[1] = zero4;
        if (tl.valid && tl.chain % p.C != 0) {               // (not the sequence's first chunk: the row exists)
            const char *pe = reinterpret_cast<const char *>(tl.baseE) + (tl.voff - rowb);
            const f4u r0 = *reinterpret_cast<const f4u *>(pe), r1 = *reinterpret_cast<const f4u *>(pe + 64);
            X32 raw;
            raw.t[0] = (f4){r0.x, r0.y, r0.z, r0.w};
            raw.t[1] = (f4){r1.x, r1.y, r1.z, r1.w};
            ep = clamp32(raw, bd);
        }
        const float dn = dot32(ep, Rv);
        c = fmaxf(c, dn > 0.f ? dot32(ep, Gv) * __builtin_amdgcn_rcpf(dn) : 0.f);
        if (g == 0 && tl.valid) phi[tl.chain] = c;
    }
}

// need[seq] = 1: the serial kernels (hmm_midq.inc) compute this sequence — its model is not served by the
// chunked scan, or its certificate (phi summed over its chunks: psi of the posterior, the one-directional CERT /
// CERT3 sums of hmm_forward / hmm_backward) is above EXACT_DELTA, or a reduce marked one of its chains: the
// operator columns went through the denormal range, or every column met an observation it survives at the emission
// floor only.  The sparse reduce keeps that mark in the pad lane of the exponent row (rows of W ints; 29 < W
// states), the dense reduces in risk[chain] (any q up to W).
__global__ __launch_bounds__(256) void k32_select(const int *__restrict__ elig, const float *__restrict__ phi,
                                                  int *__restrict__ need, int *__restrict__ nex, Plan p, float eps,
                                                  int exact_mode, const int *__restrict__ exps, const int *__restrict__ risk,
                                                  int W) {
    const int seq = blockIdx.x * 256 + threadIdx.x;
    if (seq >= p.NB) return;
    const int el = elig[seq / p.b];
    bool f = el == 0;
    if (!f && phi && exact_mode == HMM_EXACT_AUTO) {
        float s = 0.f;
        for (int c = 0; c < p.C; ++c) s += phi[(size_t)seq * p.C + c];
        f = !(s <= EXACT_DELTA);
    }
    if (!f && exact_mode == HMM_EXACT_AUTO) {
        const bool dense = el == ID_DENSE32 || el == ID_DENSE64;
        for (int c = 0; c < p.C; ++c) {
            const size_t chain = (size_t)seq * p.C + c;
            f = f || (dense ? risk[chain] != 0 : exps[chain * W + W - 1] != 0);
        }
    }
    need[seq] = f ? 1 : 0;
    if (f) atomicAdd(nex, 1);
}

// ---- dense reduce for 17..32 states: one wave per (sequence, chunk), the operator X (32 x 32) as 2 x 2 MFMA
// tiles — X[r][c]: lane (g, n) holds rows 16 r + 4g .. + 3 of column 16 c + n —, a step X <- diag(E_t) A^T X is
// eight 16x16x16 block products (32 v_mfma_f32_16x16x4_f32), columns rescaled by exact powers of two with an
// integer exponent per column, exactly as k_reduce does for 16 states.  2 q^3 flop per position: at b = 1024 x
// L = 1e5 that alone is ~45 ms and no better than one wave per sequence (hmm_midq.inc, latency-bound whatever the
// batch), but the serial kernels take their ~66 ms for 16 sequences as for 1024, and this scales with the work.
__global__ __launch_bounds__(256) void k32_reduce_dense(const float *__restrict__ A, const float *__restrict__ E,
                                                        float *__restrict__ ops, int *__restrict__ exps,
                                                        int *__restrict__ riskv, const int *__restrict__ elig, Plan p,
                                                        float eps) {
    const int lane = threadIdx.x & 63, g = lane >> 4, n = lane & 15;
    const int q = p.q;
    const long long stride = (long long)gridDim.x * 4;
    for (long long chain = (long long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
         chain < p.nchains; chain += stride) {
        const int seq = (int)(chain / p.C), c = (int)(chain - (long long)seq * p.C);
        const int m = seq / p.b;
        if (elig[m] != ID_DENSE32) continue;
        const int t0 = c * p.T;
        const int len = min(p.T, p.L - t0);
        A32 a;
        load_A32(A + (size_t)m * q * q, q, g, n, a);
        const B32 bd = make_bounds32(g, q, eps);
        const float *base = E + ((size_t)seq * p.L + t0) * q;
        const __amdgpu_buffer_rsrc_t rs = make_rsrc(base, (unsigned long long)len * q * sizeof(float));
        const int rowb = q * (int)sizeof(float);
        int voff = g * 16;
        X32 X[2];                                   // X[cb]: the two row tiles of column block cb
#pragma unroll
        for (int cb = 0; cb < 2; ++cb)
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                f4 v;
                v.x = 16 * r + 4 * g + 0 == 16 * cb + n ? 1.f : 0.f;
                v.y = 16 * r + 4 * g + 1 == 16 * cb + n ? 1.f : 0.f;
                v.z = 16 * r + 4 * g + 2 == 16 * cb + n ? 1.f : 0.f;
                v.w = 16 * r + 4 * g + 3 == 16 * cb + n ? 1.f : 0.f;
                X[cb].t[r] = v;
            }
        int ex[2] = {0, 0};                         // column 16 cb + n holds X[:, .] * 2^-ex[cb]
        // risk: EVERY column lost more than 2^-45 in ONE step — an observation that everything survives at the emission floor
        // only —, or a column's sum went below 2^-100 (the denormal range: reduce_sparse_wave's `risk`).  Such sequences
        // go to the serial kernels (the mark: riskv[chain], read by k32_select).  The exponent is clamped at -100 so that
        // the factor stays finite for a column in the denormal range.
        bool risk = false;
        auto rescale = [&]() {
            bool kept = false;                      // some column lost less than 2^-45 in this step
#pragma unroll
            for (int cb = 0; cb < 2; ++cb) {
                const float sden = sum32(X[cb]);
                risk = risk || (16 * cb + n < q && sden < 0x1p-100f);
                const int xe = max(__builtin_amdgcn_frexp_expf(sden), -100);
                kept = kept || (16 * cb + n < q && !(xe < -45));
                const float sc = __builtin_amdgcn_ldexpf(1.0f, -xe);
                X[cb].t[0] = X[cb].t[0] * sc;
                X[cb].t[1] = X[cb].t[1] * sc;
                ex[cb] += xe;
            }
            risk = risk || __builtin_amdgcn_ballot_w64(kept) == 0ull;      // EVERY column, whatever the start state
        };
        int t = 0;
        if (c == 0 && p.seq_start) {                // first observation of the sequence: no transition
            X32 e0[1];
            ld_rows32<1>(rs, voff, rowb, e0);
            const X32 ec = clamp32(e0[0], bd);
#pragma unroll
            for (int cb = 0; cb < 2; ++cb) { X[cb].t[0] = X[cb].t[0] * ec.t[0]; X[cb].t[1] = X[cb].t[1] * ec.t[1]; }
            rescale();
            voff += rowb;
            t = 1;
        }
        constexpr int PF = 4;                       // emission rows in flight ahead of the recurrence
        X32 en[PF];
        ld_rows32<PF>(rs, voff, rowb, en);
        for (; t < len; t += PF) {
            X32 ec[PF];
#pragma unroll
            for (int u = 0; u < PF; ++u) ec[u] = en[u];
            voff += PF * rowb;
            ld_rows32<PF>(rs, voff, rowb, en);
#pragma unroll
            for (int u = 0; u < PF; ++u) {
                if (t + u < len) {                  // wave-uniform
                    const X32 e = clamp32(ec[u], bd);
#pragma unroll
                    for (int cb = 0; cb < 2; ++cb) {
                        const X32 d = matvec32(a.f, X[cb]);
                        X[cb].t[0] = d.t[0] * e.t[0];
                        X[cb].t[1] = d.t[1] * e.t[1];
                    }
                    rescale();
                }
            }
        }
        float *o = ops + (size_t)chain * Q32 * Q32;
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) {
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                o[(16 * r + 4 * g + 0) * Q32 + 16 * cb + n] = X[cb].t[r].x;
                o[(16 * r + 4 * g + 1) * Q32 + 16 * cb + n] = X[cb].t[r].y;
                o[(16 * r + 4 * g + 2) * Q32 + 16 * cb + n] = X[cb].t[r].z;
                o[(16 * r + 4 * g + 3) * Q32 + 16 * cb + n] = X[cb].t[r].w;
            }
            if (g == 0) exps[(size_t)chain * Q32 + 16 * cb + n] = 16 * cb + n < q ? ex[cb] : 0;
        }
        const bool mark = __builtin_amdgcn_ballot_w64(risk) != 0ull;
        if (lane == 0) riskv[chain] = mark ? 1 : 0;
    }
}
