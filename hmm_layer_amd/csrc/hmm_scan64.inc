// hmm_scan64.inc — the chunked (time-parallel) scan for 33..64 states, included by hmm_engine.hip after
// hmm_scan32.inc.
//
// Models of this range (GenePredMultiHMMTransitioner(k = 3): 43 states, k = 4: 57,
// hmm_layer/gene_pred_hmm_transitioner.py:263-308; any learned dense A) ran one dependent chain per sequence
// (hmm_midq.inc): 60-90 ms for L = 1e5 whether the batch holds one sequence or a thousand.  For FEW sequences the
// three phases of the main pipeline pay again, with 64-state tiles:
//
//   reduce   k64_reduce_dense: one wave per (sequence, chunk), the operator X (64 x 64) as 4 x 4 MFMA tiles, a step
//            X <- diag(E_t) A^T X = 64 block products (256 v_mfma_f32_16x16x4_f32), columns rescaled by exact powers
//            of two — k_reduce for 16 states, sixty-four times over: 2 q^3 flop per position, MFMA-bound
//   scan     k64_scan: chunk-level prefix / suffix hops over 64 x 64 operators, one wave per direction, lane = state
//   apply    k64_forward / k64_backward: FOUR 16-state tile rows per chain (a step's mat-vec is sixteen 16x16x16
//            block products), the cell's exact step, alpha_hat checkpoints every 2 steps, the clamp flags of psi in
//            the sign bits (backward_body in hmm_engine.hip); the forward operands of A live in registers, the
//            backward ones in LDS (one wave per SIMD either way)
//
// The reduce costs 8x what the 32-state one does, so the path is taken for up to SCAN64_MAX_SEQ sequences per call
// (scan64_wanted) and only for models whose support is primitive (k64_check, B^4096 > 0: Wielandt's (q-1)^2 + 1 =
// 3970 for q = 64); everything else — larger batches, reducible models, sequences whose psi is above EXACT_DELTA —
// is served by the one-wave-per-sequence kernels, which take a per-sequence mask.  hmm_posterior (all modes),
// hmm_forward and hmm_backward; gradients and Viterbi stay on hmm_midq.inc.  This file holds the kernels; the plan
// (MidPlan) and the host drivers (scan_*<Scan64>) are shared with the 32-state rows: hmm_scan_mid.inc.

#define Q64 64
#define SUB64 2                       // steps per apply block = checkpoint spacing
#define OUT64_ROWS 4                  // rows per chain staged in LDS per flush
#define OUT64_STRIDE (OUT64_ROWS * Q64 + 4)
#define OUT64_SEG (16 * OUT64_STRIDE + 32)
#define SCAN64_MAX_SEQ 96             // sequences per call up to which 33..64 states take the chunked path
#define SCAN64_MIN_LEN 256
#define SCAN64_SPARSE_MAX_SEQ 56     // ... for sparse models (see k64_check)

static bool scan64_wanted(int k, int b, int L, int q) {
    return q > Q32 && q <= Q64 && (long long)k * b <= SCAN64_MAX_SEQ && L >= SCAN64_MIN_LEN;
}

// elig[m]: ID_DENSE64 = the chunked scan serves this model (primitive support), 0 = the serial kernels do
__global__ __launch_bounds__(64) void k64_check(const float *__restrict__ A, int *__restrict__ elig, int q,
                                                int exact_mode, float eps, int *__restrict__ nex, int nseq, int force_dense) {
    const int m = blockIdx.x, lane = threadIdx.x;
    const float *Am = A + (size_t)m * q * q;
    if (m == 0 && lane == 0) *nex = 0;
    bool bad = exact_mode == HMM_EXACT_ALWAYS || exact_mode == HMM_EXACT_ALWAYS_NARROW;
    // A SPARSE model (no state with more than MQ_SP_MAX predecessors or successors: the multi-copy gene models) walks a
    // sequence of 1e5 in ~30 ms on the one-wave-per-sequence kernels whatever the batch (hmm_midq.inc's sparse step),
    // the dense 64-state reduce costs ~0.5 ms per sequence: above SCAN64_SPARSE_MAX_SEQ sequences they have it
    if (!bad && exact_mode == HMM_EXACT_AUTO && nseq > SCAN64_SPARSE_MAX_SEQ && !force_dense) {
        int nin = 0, nout = 0;
        if (lane < q)
            for (int i = 0; i < q; ++i) {
                nin += Am[(size_t)i * q + lane] != 0.f ? 1 : 0;
                nout += Am[(size_t)lane * q + i] != 0.f ? 1 : 0;
            }
        bad = __ballot(nin > MQ_SP_MAX || nout > MQ_SP_MAX) == 0ull;
    }
    if (!bad && exact_mode == HMM_EXACT_AUTO) {
        unsigned long long row = 0;
        if (lane < q)
            for (int j = 0; j < q; ++j) row |= (Am[lane * q + j] > eps) ? (1ull << j) : 0ull;
        for (int it = 0; it < 12; ++it) {
            unsigned long long nr = 0;
            for (int j = 0; j < q; ++j) {
                const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)row, j);
                const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(row >> 32), j);
                nr |= ((row >> j) & 1ull) ? (((unsigned long long)hi << 32) | lo) : 0ull;
            }
            row = nr;
        }
        const unsigned long long full = q >= 64 ? ~0ull : ((1ull << q) - 1ull);
        bad = __ballot(lane < q && row != full) != 0ull;
    }
    if (lane == 0) elig[m] = bad ? 0 : ID_DENSE64;
}

// ---- 64-state vectors in the tile layout: lane (g, n) holds states 16 t + 4g .. + 3 of chain n in t[t]
struct X64 { f4 t[4]; };
struct A64 { f4 a[4][4]; };           // MFMA A-operands of one direction: block (r, c), the lane's four k values

__device__ __forceinline__ void load_A64(const float *A, int q, int g, int n, bool fwd, A64 &a) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            float v[4];
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                const int s = 16 * c + 4 * g + kk, d = 16 * r + n;       // contraction index, output row
                const bool ok = s < q && d < q;
                v[kk] = ok ? (fwd ? A[s * q + d] : A[d * q + s]) : 0.f;   // alpha' = A^T alpha | R = A bh
            }
            a.a[r][c] = (f4){v[0], v[1], v[2], v[3]};
        }
}
__device__ __forceinline__ X64 matvec64(const A64 &a, const X64 &x) {
    X64 d;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        f4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < 4; ++c) acc = mfma4v(a.a[r][c], x.t[c], acc);
        d.t[r] = acc;
    }
    return d;
}
// the same with the operands in LDS: la[(r * 4 + c) * 64 + lane]
__device__ __forceinline__ X64 matvec64_lds(const f4 *la, int lane, const X64 &x) {
    X64 d;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        f4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < 4; ++c) acc = mfma4v(la[(r * 4 + c) * 64 + lane], x.t[c], acc);
        d.t[r] = acc;
    }
    return d;
}
__device__ __forceinline__ float sum64(const X64 &x) {
    return col_sum((hsum(x.t[0]) + hsum(x.t[1])) + (hsum(x.t[2]) + hsum(x.t[3])));
}
__device__ __forceinline__ float sum64_abs(const X64 &x) {
    return col_sum((hsum_abs(x.t[0]) + hsum_abs(x.t[1])) + (hsum_abs(x.t[2]) + hsum_abs(x.t[3])));
}
struct B64 { Bounds t[4]; };
__device__ __forceinline__ B64 make_bounds64(int g, int q, float eps) {
    B64 b;
    const float inf = __builtin_inff();
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int s0 = 16 * t + 4 * g;
        b.t[t].lo.x = s0 + 0 < q ? eps : 0.f;  b.t[t].hi.x = s0 + 0 < q ? inf : 0.f;
        b.t[t].lo.y = s0 + 1 < q ? eps : 0.f;  b.t[t].hi.y = s0 + 1 < q ? inf : 0.f;
        b.t[t].lo.z = s0 + 2 < q ? eps : 0.f;  b.t[t].hi.z = s0 + 2 < q ? inf : 0.f;
        b.t[t].lo.w = s0 + 3 < q ? eps : 0.f;  b.t[t].hi.w = s0 + 3 < q ? inf : 0.f;
    }
    return b;
}
// emission rows: four 16-byte loads per row; what lies past the row's q states is the next row (or, at the
// tensor's end, outside the descriptor: 0) and is zeroed by the clamp bounds
template <int N>
__device__ __forceinline__ void ld_rows64(__amdgpu_buffer_rsrc_t r, int voff, int rowb, X64 (&e)[N]) {
#pragma unroll
    for (int s = 0; s < N; ++s)
#pragma unroll
        for (int t = 0; t < 4; ++t)
            e[s].t[t] = __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(r, voff + s * rowb + 64 * t, 0, 0));
}
__device__ __forceinline__ X64 clamp64(const X64 &e, const B64 &b) {
    X64 r;
#pragma unroll
    for (int t = 0; t < 4; ++t) r.t[t] = clampE(e.t[t], b.t[t]);
    return r;
}
__device__ __forceinline__ X64 ld_vec64(const float *v, int g) {
    X64 r;
#pragma unroll
    for (int t = 0; t < 4; ++t) r.t[t] = *reinterpret_cast<const f4 *>(v + 16 * t + 4 * g);
    return r;
}

// output rows staged in wave-private LDS and flushed as 16-byte pieces (Out32 of hmm_scan32.inc for rows of up to 64)
struct Out64 { float *seg; char *base; int q; };
__device__ __forceinline__ Out64 make_out64(float *seg, char *base, int q, int lane, int voff0, int len) {
    Out64 o = {seg, base, q};
    int *tab = reinterpret_cast<int *>(seg + 16 * OUT64_STRIDE);
    if (lane < 16) { tab[lane] = voff0; tab[16 + lane] = len; }
    __builtin_amdgcn_wave_barrier();
    return o;
}
__device__ __forceinline__ void stage64(const Out64 &o, int n, int g, int srow, const X64 &v) {
    float *pr = o.seg + n * OUT64_STRIDE + srow * o.q;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int s0 = 16 * t + 4 * g;
        if (s0 + 0 < o.q) pr[s0 + 0] = v.t[t].x;
        if (s0 + 1 < o.q) pr[s0 + 1] = v.t[t].y;
        if (s0 + 2 < o.q) pr[s0 + 2] = v.t[t].z;
        if (s0 + 3 < o.q) pr[s0 + 3] = v.t[t].w;
    }
}
__device__ __forceinline__ void flush64(const Out64 &o, int lane, int row0, int nrows) {
    const int *tab = reinterpret_cast<const int *>(o.seg + 16 * OUT64_STRIDE);
    const int ppc = nrows * o.q / 4;                     // (nrows is a multiple of 4: whole 16-byte pieces)
    const float inv = 1.0f / (float)ppc;
    __builtin_amdgcn_wave_barrier();
    for (int pc = lane; pc < 16 * ppc; pc += 64) {
        const int c = (int)(((float)pc + 0.5f) * inv);
        const int kk = pc - c * ppc;
        int rows = tab[16 + c] - row0;
        rows = rows > nrows ? nrows : rows;
        const int nfl = rows * o.q - 4 * kk;
        if (nfl <= 0) continue;
        const f4 v = *reinterpret_cast<const f4 *>(o.seg + c * OUT64_STRIDE + 4 * kk);
        char *dst = o.base + tab[c] + (row0 * o.q + 4 * kk) * (int)sizeof(float);
        if (nfl >= 4) { __builtin_nontemporal_store(v, reinterpret_cast<f4u *>(dst)); }
        else if (nfl == 3) { P3 t = {v.x, v.y, v.z}; *reinterpret_cast<P3 *>(dst) = t; }
        else if (nfl == 2) { P2 t = {v.x, v.y}; *reinterpret_cast<P2 *>(dst) = t; }
        else { *reinterpret_cast<float *>(dst) = v.x; }
    }
    __builtin_amdgcn_wave_barrier();
}

// ---- dense reduce: one wave per (sequence, chunk); X[cb].t[r]: rows 16 r + 4g .. + 3 of column 16 cb + n
__global__ __launch_bounds__(256) void k64_reduce_dense(const float *__restrict__ A, const float *__restrict__ E,
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
        if (elig[m] != ID_DENSE64) continue;
        const int t0 = c * p.T;
        const int len = min(p.T, p.L - t0);
        A64 a;
        load_A64(A + (size_t)m * q * q, q, g, n, true, a);
        const B64 bd = make_bounds64(g, q, eps);
        const float *base = E + ((size_t)seq * p.L + t0) * q;
        const __amdgpu_buffer_rsrc_t rs = make_rsrc(base, (unsigned long long)len * q * sizeof(float));
        const int rowb = q * (int)sizeof(float);
        int voff = g * 16;
        X64 X[4];
#pragma unroll
        for (int cb = 0; cb < 4; ++cb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                f4 v;
                v.x = 16 * r + 4 * g + 0 == 16 * cb + n ? 1.f : 0.f;
                v.y = 16 * r + 4 * g + 1 == 16 * cb + n ? 1.f : 0.f;
                v.z = 16 * r + 4 * g + 2 == 16 * cb + n ? 1.f : 0.f;
                v.w = 16 * r + 4 * g + 3 == 16 * cb + n ? 1.f : 0.f;
                X[cb].t[r] = v;
            }
        int ex[4] = {0, 0, 0, 0};
        bool risk = false;                           // -> riskv[chain]: see k32_reduce_dense
        auto rescale = [&]() {
            bool kept = false;
#pragma unroll
            for (int cb = 0; cb < 4; ++cb) {
                const float sden = sum64(X[cb]);
                risk = risk || (16 * cb + n < q && sden < 0x1p-100f);
                const int xe = max(__builtin_amdgcn_frexp_expf(sden), -100);
                kept = kept || (16 * cb + n < q && !(xe < -45));
                const float sc = __builtin_amdgcn_ldexpf(1.0f, -xe);
#pragma unroll
                for (int r = 0; r < 4; ++r) X[cb].t[r] = X[cb].t[r] * sc;
                ex[cb] += xe;
            }
            risk = risk || __builtin_amdgcn_ballot_w64(kept) == 0ull;
        };
        int t = 0;
        if (c == 0 && p.seq_start) {                // first observation of the sequence: no transition
            X64 e0[1];
            ld_rows64<1>(rs, voff, rowb, e0);
            const X64 ec = clamp64(e0[0], bd);
#pragma unroll
            for (int cb = 0; cb < 4; ++cb)
#pragma unroll
                for (int r = 0; r < 4; ++r) X[cb].t[r] = X[cb].t[r] * ec.t[r];
            rescale();
            voff += rowb;
            t = 1;
        }
        X64 en[1];
        ld_rows64<1>(rs, voff, rowb, en);
        for (; t < len; ++t) {
            const X64 e = clamp64(en[0], bd);
            voff += rowb;
            ld_rows64<1>(rs, voff, rowb, en);       // (past the chunk: outside the descriptor, zeros)
#pragma unroll
            for (int cb = 0; cb < 4; ++cb) {
                const X64 d = matvec64(a, X[cb]);
#pragma unroll
                for (int r = 0; r < 4; ++r) X[cb].t[r] = d.t[r] * e.t[r];
            }
            rescale();
        }
        float *o = ops + (size_t)chain * Q64 * Q64;
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                o[(16 * r + 4 * g + 0) * Q64 + 16 * cb + n] = X[cb].t[r].x;
                o[(16 * r + 4 * g + 1) * Q64 + 16 * cb + n] = X[cb].t[r].y;
                o[(16 * r + 4 * g + 2) * Q64 + 16 * cb + n] = X[cb].t[r].z;
                o[(16 * r + 4 * g + 3) * Q64 + 16 * cb + n] = X[cb].t[r].w;
            }
            if (g == 0) exps[(size_t)chain * Q64 + 16 * cb + n] = 16 * cb + n < q ? ex[cb] : 0;
        }
        const bool mark = __builtin_amdgcn_ballot_w64(risk) != 0ull;
        if (lane == 0) riskv[chain] = mark ? 1 : 0;
    }
}

// ---- scan over 64 x 64 chunk operators: ops[chain][i][k], column k scaled by 2^-exps[k].  One 128-thread block per
// sequence, wave 0 the forward prefix chain, wave 1 the backward suffix chain; lane = state.
__global__ __launch_bounds__(128) void k64_scan(const float *__restrict__ pi, const float *__restrict__ ops,
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
    if (dir == 0) {
        const float praw = act ? pi[(size_t)m * q + lane] : 0.f;
        float a = act ? fmaxf(praw, eps) : 0.f;
        double ll = 0.0;
        prefix[chain0 * Q64 + lane] = praw;
        if (lane == 0) llpre[chain0] = 0.0;
        for (int c = 0; c < C; ++c) {
            const f4 *row = reinterpret_cast<const f4 *>(ops + (chain0 + c) * Q64 * Q64 + lane * Q64);
            const int xec = exps[(chain0 + c) * Q64 + lane];
            const int we = (a > 0.f) ? __builtin_amdgcn_frexp_expf(a) + xec : -(1 << 28);
            const int emax = wave_max32(we);
            int sh = xec - emax;
            sh = sh < -300 ? -300 : sh;
            const float w = __builtin_amdgcn_ldexpf(a, sh);
            float acc = 0.f;
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                const f4 r4 = row[u];
                acc = fmaf(r4.x, lane_bcast(w, 4 * u + 0), acc);
                acc = fmaf(r4.y, lane_bcast(w, 4 * u + 1), acc);
                acc = fmaf(r4.z, lane_bcast(w, 4 * u + 2), acc);
                acc = fmaf(r4.w, lane_bcast(w, 4 * u + 3), acc);
            }
            acc = act ? acc : 0.f;
            const float S = wave_sum32(acc);
            a = acc / S;
            ll += (double)__logf(S) + (double)emax * LN2;
            if (c + 1 < C) {
                prefix[(chain0 + c + 1) * Q64 + lane] = a;
                if (lane == 0) llpre[chain0 + c + 1] = ll;
            }
        }
        if (lane == 0) loglik[seq] = ll;
    } else {
        float v = act ? 1.f : 0.f;
        double lb = 0.0;
        for (int c = C - 1; c >= 0; --c) {
            suffix[(chain0 + c) * Q64 + lane] = v;
            if (lane == 0) lsuf[chain0 + c] = lb;
            if (c == 0) break;
            const float *X = ops + (chain0 + c) * Q64 * Q64;
            const int xec = exps[(chain0 + c) * Q64 + lane];
            float u = 0.f;
#pragma unroll 16
            for (int j = 0; j < Q64; ++j) u = fmaf(X[j * Q64 + lane], lane_bcast(v, j), u);
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

__device__ __forceinline__ float dot64(const X64 &a, const X64 &b) {
    return col_sum((hsum(a.t[0] * b.t[0]) + hsum(a.t[1] * b.t[1])) + (hsum(a.t[2] * b.t[2]) + hsum(a.t[3] * b.t[3])));
}

// ---- apply, forward.  LOGA = false, CERT = false: alpha_hat entering every SUB64-step block -> ckpt
// ([wave][block][chain][64]); LOGA = true: log alpha -> out (hmm_forward with log alpha); CERT: the clamp-born share
// -> phi[chain], k32_forward's CERT
template <bool LOGA, bool CERT = false>
__global__ __launch_bounds__(256) void k64_forward(const float *__restrict__ A, const float *__restrict__ E,
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
    A64 a;
    load_A64(A + (size_t)tl.m * q * q, q, g, n, true, a);
    const B64 bd = make_bounds64(g, q, eps);
    const int rowb = q * (int)sizeof(float);
    X64 X = ld_vec64(prefix + (size_t)tl.chain * Q64, g);
    const f4 zero4 = {0.f, 0.f, 0.f, 0.f};
    X64 Fv, Xc = X, Fc;                                      // CERT: clamp-born part of X; both at the chain's last step
#pragma unroll
    for (int t = 0; t < 4; ++t) Fv.t[t] = Fc.t[t] = zero4;
    float *ck = CKPT ? ckpt + (((size_t)wave * p.nsub) * 16 + n) * Q64 + 4 * g : nullptr;
    __shared__ __attribute__((aligned(16))) float ostage[LOGA ? 4 * OUT64_SEG : 4];
    Out64 os = {};
    if (LOGA)
        os = make_out64(ostage + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) * OUT64_SEG,
                        reinterpret_cast<char *>(out + (tl.baseE - E)), q, lane, tl.voff - g * 16, tl.len);
    double llb = LOGA ? llpre[tl.chain] : 0.0;
    constexpr int GB = OUT64_ROWS / SUB64;
    int voff = tl.voff;
    X64 en[SUB64];
    ld_rows64<SUB64>(tl.rsE, voff, rowb, en);
    for (int j = 0; j < p.nsub; ++j) {
        if (CKPT && tl.valid && j * SUB64 < tl.len) {
#pragma unroll
            for (int t = 0; t < 4; ++t) *reinterpret_cast<f4 *>(ck + (size_t)j * 16 * Q64 + 16 * t) = X.t[t];
        }
        X64 e[SUB64];
#pragma unroll
        for (int s = 0; s < SUB64; ++s) e[s] = en[s];
        if (j + 1 < p.nsub) ld_rows64<SUB64>(tl.rsE, voff + SUB64 * rowb, rowb, en);
        float lacc = 0.f;
#pragma unroll
        for (int s = 0; s < SUB64; ++s) {
            const bool init = tl.first && j == 0 && s == 0;
            const X64 ec = clamp64(e[s], bd);
            const X64 d = matvec64(a, X);
            X64 sf;
#pragma unroll
            for (int t = 0; t < 4; ++t) sf.t[t] = fmax4(sel4(init, X.t[t], d.t[t]), eps) * ec.t[t];
            const float S = sum64(sf);
            const float inv = __builtin_amdgcn_rcpf(S);
            if (CERT) {
                const X64 df = matvec64(a, Fv);
                const bool last = j * SUB64 + s + 1 == tl.len;
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    Fv.t[t] = sel4(init, Fv.t[t], born4(d.t[t], df.t[t], eps)) * ec.t[t] * inv;
                    X.t[t] = sf.t[t] * inv;
                    Xc.t[t] = sel4(last, X.t[t], Xc.t[t]);
                    Fc.t[t] = sel4(last, Fv.t[t], Fc.t[t]);
                }
            } else {
#pragma unroll
                for (int t = 0; t < 4; ++t) X.t[t] = sf.t[t] * inv;
            }
            if (LOGA) {
                lacc += (j * SUB64 + s < tl.len) ? __logf(S) : 0.f;
                const float base = (float)(llb + (double)lacc);
                X64 la;
#pragma unroll
                for (int t = 0; t < 4; ++t) la.t[t] = log4(X.t[t]) + base;
                stage64(os, n, g, (j % GB) * SUB64 + s, la);
            }
        }
        if (LOGA) {
            llb += (double)lacc;
            if ((j + 1) % GB == 0 || j + 1 == p.nsub) flush64(os, lane, (j / GB) * OUT64_ROWS, OUT64_ROWS);
        }
        voff += SUB64 * rowb;
    }
    if (CERT) {
        const X64 sv = ld_vec64(suffix + (size_t)tl.chain * Q64, g);
        float c = dot64(Fc, sv) * __builtin_amdgcn_rcpf(dot64(Xc, sv));
        if (LOGA) {                                          // (k32_forward's shmax and shnext)
            X64 en1;
#pragma unroll
            for (int t = 0; t < 4; ++t) en1.t[t] = zero4;
            const bool more = tl.valid && tl.chain % p.C != p.C - 1;
            if (more) {
                X64 r1[1];
                ld_rows64<1>(tl.rsE, tl.voff + tl.len * rowb, rowb, r1);
                en1 = clamp64(r1[0], bd);
            }
            X64 dx = matvec64(a, Xc);
            const X64 df = matvec64(a, Fc);
#pragma unroll
            for (int t = 0; t < 4; ++t) dx.t[t] = fmax4(dx.t[t], eps);
            const float dn = dot64(en1, dx);
            const float shnext = (more && dn > 0.f) ? dot64(en1, df) * __builtin_amdgcn_rcpf(dn) : 0.f;
            c = fmaxf(fmaxf(c, sum64(Fc)), shnext);
        }
        if (tl.valid && g == 0) phi[tl.chain] = c;
    }
}

// ---- apply, backward.  MODE 0: gamma, 1: log gamma, 2: log gamma + loglik, 3: log beta (no forward part).
// phi: psi per chain (backward_body in hmm_engine.hip).  A's forward operands in registers, the backward ones in LDS.
// CERT3 (MODE 3): the clamp-born share of R -> phi[chain], k32_backward's CERT3
template <int MODE, bool CERT3 = false>
__global__ __launch_bounds__(256) void k64_backward(const float *__restrict__ A, const float *__restrict__ E,
                                                    const float *__restrict__ ckpt, const float *__restrict__ suffix,
                                                    const double *__restrict__ lsuf, const double *__restrict__ loglik,
                                                    float *__restrict__ out, float *__restrict__ phi,
                                                    const int *__restrict__ elig, Plan p, float eps, long long nwaves,
                                                    const float *__restrict__ prefix = nullptr) {
    static_assert(!CERT3 || MODE == 3, "CERT3 is the log beta certificate");
    const long long wave = (long long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (wave >= nwaves) return;
    const int lane = threadIdx.x & 63, g = lane >> 4, n = lane & 15;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int q = p.q;
    const Tile32 tl = make_tile32(E, p, wave, g, n);
    if (elig[tl.m] == 0) return;
    __shared__ __attribute__((aligned(16))) f4 abl[4 * 16 * 64];          // [wave][(r, c)][lane]
    __shared__ __attribute__((aligned(16))) float ostage[4 * OUT64_SEG];
    f4 *la = abl + w * 16 * 64;
    {
        A64 ab;
        load_A64(A + (size_t)tl.m * q * q, q, g, n, false, ab);
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) la[(r * 4 + c) * 64 + lane] = ab.a[r][c];
        __builtin_amdgcn_wave_barrier();
    }
    A64 af;
    if (MODE != 3) load_A64(A + (size_t)tl.m * q * q, q, g, n, true, af);
    const B64 bd = make_bounds64(g, q, eps);
    const int rowb = q * (int)sizeof(float);
    float *seg = ostage + w * OUT64_SEG;
    const Out64 os = make_out64(seg, reinterpret_cast<char *>(out + (tl.baseE - E)), q, lane, tl.voff - g * 16, tl.len);

    X64 Rv = ld_vec64(suffix + (size_t)tl.chain * Q64, g);
    float llf = 0.f;
    if (MODE == 2) llf = (float)loglik[tl.chain / p.C];
    double lbb = MODE == 3 ? lsuf[tl.chain] : 0.0;
    const float *ck = MODE == 3 ? nullptr : ckpt + (((size_t)wave * p.nsub) * 16 + n) * Q64 + 4 * g;
    float psacc = 0.f;
    const f4 zero4 = {0.f, 0.f, 0.f, 0.f};
    X64 Gv, Rc = Rv, Gc, ec0;                                // CERT3: clamp-born part of R; R, Gv, E at the first position
#pragma unroll
    for (int t = 0; t < 4; ++t) Gv.t[t] = Gc.t[t] = ec0.t[t] = zero4;
    constexpr int GB = OUT64_ROWS / SUB64;
    for (int j = p.nsub - 1; j >= 0; --j) {
        const int srow = (j % GB) * SUB64;
        X64 e[SUB64];
        ld_rows64<SUB64>(tl.rsE, tl.voff + j * SUB64 * rowb, rowb, e);
#pragma unroll
        for (int s = 0; s < SUB64; ++s) e[s] = clamp64(e[s], bd);
        X64 fa[SUB64];
        if (MODE != 3) {
            X64 X;
#pragma unroll
            for (int t = 0; t < 4; ++t)
                X.t[t] = (tl.valid && j * SUB64 < tl.len) ? *reinterpret_cast<const f4 *>(ck + (size_t)j * 16 * Q64 + 16 * t) : zero4;
#pragma unroll
            for (int s = 0; s < SUB64; ++s) {
                const bool init = tl.first && j == 0 && s == 0;
                const X64 d = matvec64(af, X);
                X64 sf;
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    sf.t[t] = sel4(init, fmax4(X.t[t], eps), clamp_flag4(d.t[t], eps)) * e[s].t[t];
                const float inv = __builtin_amdgcn_rcpf(sum64_abs(sf));
#pragma unroll
                for (int t = 0; t < 4; ++t) { fa[s].t[t] = sf.t[t] * inv; X.t[t] = abs4(fa[s].t[t]); }
            }
        }
        float lacc = 0.f;
#pragma unroll
        for (int s = SUB64 - 1; s >= 0; --s) {
            const bool act = j * SUB64 + s < tl.len;
            X64 gm;
            if (MODE == 3) {
                const float base = (float)(lbb + (double)lacc);
#pragma unroll
                for (int t = 0; t < 4; ++t) gm.t[t] = log4(Rv.t[t]) + base;
            } else {
#pragma unroll
                for (int t = 0; t < 4; ++t) gm.t[t] = fa[s].t[t] * Rv.t[t];        // negative: exactly one clamp was active
                const float Sg = sum64_abs(gm);
                const float ig = __builtin_amdgcn_rcpf(Sg);
                psacc = fmaf((hsum_neg(gm.t[0]) + hsum_neg(gm.t[1])) + (hsum_neg(gm.t[2]) + hsum_neg(gm.t[3])), act ? ig : 0.f, psacc);
                if (MODE == 0) {
#pragma unroll
                    for (int t = 0; t < 4; ++t) gm.t[t] = mul_abs4(gm.t[t], f4{ig, ig, ig, ig});
                } else {
                    const float lg = __logf(Sg) - llf;
#pragma unroll
                    for (int t = 0; t < 4; ++t) gm.t[t] = log4(abs4(gm.t[t])) - lg;
                }
            }
            stage64(os, n, g, srow + s, gm);
            if (CERT3 && s == 0) { Rc = Rv; Gc = Gv; ec0 = e[0]; }      // (the last block executed is the chunk's first)
            X64 sf;
#pragma unroll
            for (int t = 0; t < 4; ++t) sf.t[t] = MODE == 3 ? e[s].t[t] * Rv.t[t] : mul_abs4(Rv.t[t], e[s].t[t]);
            const float Sb = sum64(sf);
            if (MODE == 3) lacc += act ? __logf(Sb) : 0.f;
            const float ib = __builtin_amdgcn_rcpf(Sb);
#pragma unroll
            for (int t = 0; t < 4; ++t) sf.t[t] = sf.t[t] * ib;
            const X64 d = matvec64_lds(la, lane, sf);
            if (CERT3) {
                X64 gs;
#pragma unroll
                for (int t = 0; t < 4; ++t) gs.t[t] = e[s].t[t] * Gv.t[t] * ib;
                const X64 ug = matvec64_lds(la, lane, gs);
#pragma unroll
                for (int t = 0; t < 4; ++t) Gv.t[t] = sel4(act, born4(d.t[t], ug.t[t], eps), Gv.t[t]);
            }
#pragma unroll
            for (int t = 0; t < 4; ++t)
                Rv.t[t] = sel4(act, MODE == 3 ? fmax4(d.t[t], eps) : clamp_flag4(d.t[t], eps), Rv.t[t]);
        }
        if (MODE == 3) lbb += (double)lacc;
        if (j % GB == 0) flush64(os, lane, j * SUB64, OUT64_ROWS);
    }
    psacc = col_sum(psacc);
    if (MODE != 3 && g == 0 && tl.valid) phi[tl.chain] = psacc;
    if (CERT3) {                                             // (k32_backward's CERT3)
        A64 afc;
        load_A64(A + (size_t)tl.m * q * q, q, g, n, true, afc);
        const X64 P = ld_vec64(prefix + (size_t)tl.chain * Q64, g);
        const X64 dp = matvec64(afc, P);
        X64 a0;
#pragma unroll
        for (int t = 0; t < 4; ++t) a0.t[t] = fmax4(sel4(tl.first, P.t[t], dp.t[t]), eps) * ec0.t[t];
        float c = dot64(a0, Gc) * __builtin_amdgcn_rcpf(dot64(a0, Rc));
        c = fmaxf(c, sum64(Gv) * __builtin_amdgcn_rcpf(sum64(Rv)));
        X64 ep;
#pragma unroll
        for (int t = 0; t < 4; ++t) ep.t[t] = zero4;
        if (tl.valid && tl.chain % p.C != 0) {
            const char *pe = reinterpret_cast<const char *>(tl.baseE) + (tl.voff - rowb);
            X64 raw;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const f4u r = *reinterpret_cast<const f4u *>(pe + 64 * t);
                raw.t[t] = (f4){r.x, r.y, r.z, r.w};
            }
            ep = clamp64(raw, bd);
        }
        const float dn = dot64(ep, Rv);
        c = fmaxf(c, dn > 0.f ? dot64(ep, Gv) * __builtin_amdgcn_rcpf(dn) : 0.f);
        if (g == 0 && tl.valid) phi[tl.chain] = c;
    }
}
