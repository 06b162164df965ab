// hmm_scan_rows.inc — the chunked (time-parallel) scan for 17..64 states, included by hmm_engine.hip.
//
// Models of this range do not fit the 16-state MFMA tile of the main pipeline and ran one dependent chain per
// sequence (hmm_midq.inc: 60-90 ms for L = 1e5 whether the batch holds one sequence or a thousand).  Here they get
// the same three phases with rows of NT 16-state tiles per chain, NT = 2 (17..32 states: the 29-state two-copy gene
// model, hmm_layer/gene_pred_hmm_transitioner.py:263-308, GenePredMultiHMMTransitioner(k = 2)) or NT = 4 (33..64
// states: k = 3 with 43 states, k = 4 with 57, any learned dense A).  Every helper and kernel below is written once,
// templated over NT; what differs between the widths is a constant or a named policy in Rows<NT>.
//
//   reduce   reduce_dense<NT>: one wave per (sequence, chunk), the operator X (W x W) as NT x NT MFMA tiles, a step
//            X <- diag(E_t) A^T X = NT^3 16x16x16 block products, columns rescaled by exact powers of two —
//            k_reduce for 16 states, NT^3 times over: 2 q^3 flop per position.  The compiled 29-state topology
//            has its own sparse reduce (k_reduce_sparse_wide<TopoGene29>: 32 lanes per chain, 45 structural fma's)
//   scan     scan<NT>: chunk-level prefix / suffix hops over W x W operators, one wave per direction (from given entry
//            vectors for a time slab of a sequence-sharded call; compose<NT> forms a slab's operator: hmm_seqshard_mid.inc)
//   apply    forward<NT> / backward<NT>: NT tile rows per chain (a W-state vector is NT tile rows; a step's
//            mat-vec is NT^2 block products), the cell's exact step, alpha_hat checkpoints every BLK steps, the
//            clamp flags of psi in the sign bits (backward_body in hmm_engine.hip), posteriors staged in LDS
//
// Which models take this path is decided on the device (k32_check / k64_check): the support of A must be primitive,
// and the 64-state rows, whose reduce costs 8x what the 32-state one does, serve only few long sequences
// (scan64_wanted).  Everything else — reducible models, larger batches of 33..64 states, and sequences whose
// certificate (psi, or the one-directional CERT / CERT3 sums) fires or that a reduce marked (k_scan_select) — is
// served by the one-wave-per-sequence kernels of hmm_midq.inc, which implement the cell's serial semantics exactly
// and take a per-sequence mask.  hmm_posterior (all modes), hmm_forward and hmm_backward use this path; the gradients
// run per chunk of this plan (hmm_postgrad_chunked.inc, hmm_grad_scan.inc, hmm_postgrad_scan.inc), otherwise — and Viterbi always — on
// hmm_midq.inc.  This file holds the kernels; the plan (MidPlan) and the host drivers are in hmm_scan_mid.inc.

#define Q32 32
#define Q64 64
#define SCAN64_MAX_SEQ 96             // sequences per call up to which 33..64 states take the chunked path
#define SCAN64_MIN_LEN 256
#define SCAN64_SPARSE_MAX_SEQ 56      // ... for sparse models (see k64_check)

// the constants of a row width, and where the two widths' kernels differ in structure (chosen for register
// pressure: the 64-state apply kernels and the 64-state reduce run one wave per SIMD at up to 256 VGPRs)
template <int NT>
struct Rows {
    static_assert(NT == 2 || NT == 4, "rows of 32 or 64 states");
    static constexpr int W = 16 * NT;
    static constexpr int BLK = NT == 2 ? 4 : 2;               // steps per apply block = checkpoint spacing
    static constexpr int STAGE_ROWS = NT == 2 ? 8 : 4;        // rows per chain staged in LDS per flush
    static constexpr int STAGE_STRIDE = STAGE_ROWS * W + 4;
    static constexpr int STAGE_SEG = 16 * STAGE_STRIDE + 32;  // 16 chains, then the chain table [voff x 16][len x 16]
    // elig[m] of a model on the chunked scan with the dense MFMA reduce (TopoGene29::ID (| TOPO_UNIT): with the
    // compiled sparse reduce; 0: the serial kernels serve the model)
    static constexpr int ID_DENSE = NT == 2 ? 4 : 5;
    // reduce_dense: emission rows in flight ahead of the recurrence (64: the operator alone fills the 256 VGPRs)
    static constexpr int REDUCE_PF = NT == 2 ? 4 : 1;
    // scan: the next operator's row / column in registers one hop ahead (64: 64 more VGPRs would halve the waves
    // per SIMD; lane = state, loads at the point of use)
    static constexpr bool SCAN_PREFETCH = NT == 2;
    // backward: the next block's emission rows and checkpoint in flight during this block (64: no room)
    static constexpr bool BWD_PREFETCH = NT == 2;
    // backward: A's backward operands in LDS, the forward set reloaded for the CERT3 tail (32: both in registers)
    static constexpr bool BWD_A_LDS = NT == 4;
};
__host__ __device__ inline bool elig_dense(int el) { return el == Rows<2>::ID_DENSE || el == Rows<4>::ID_DENSE; }

static bool scan64_wanted(int k, int b, int L, int q) {
    return q > Q32 && q <= Q64 && (long long)k * b <= SCAN64_MAX_SEQ && L >= SCAN64_MIN_LEN;
}

// elig[m] for 17..32 states: 0 = the serial kernels serve this model (support not primitive, or the routing is
// forced); TopoGene29::ID (| TOPO_UNIT) = the chunked scan with the compiled sparse reduce; Rows<2>::ID_DENSE = the
// chunked scan with the dense MFMA reduce (any other primitive model of 17..32 states: a learned dense A, other
// topologies).  One wave per model.
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
    if (lane == 0) elig[m] = bad ? 0 : (out29 ? Rows<2>::ID_DENSE : (T::ID | (nonunit ? 0 : TOPO_UNIT)));
}

// elig[m] for 33..64 states: Rows<4>::ID_DENSE = the chunked scan serves this model (primitive support: B^4096 > 0,
// Wielandt's (q-1)^2 + 1 = 3970 for q = 64), 0 = the serial kernels do
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
    if (lane == 0) elig[m] = bad ? 0 : Rows<4>::ID_DENSE;
}

// ---- W-state vectors in the tile layout: lane (g, n) holds states 16 t + 4g .. + 3 of chain n in t[t].  A step's
// mat-vec is NT x NT 16x16x16 block products: D[r] = sum_c Aop[r][c] * X[c].
template <int NT> struct XT { f4 t[NT]; };
template <int NT> struct AT { f4 a[NT][NT]; };      // MFMA A-operands of one direction: block (r, c), the lane's four k values
template <int NT> struct BT { Bounds t[NT]; };

template <int NT>
__device__ __forceinline__ void load_A(const float *A, int q, int g, int n, bool fwd, AT<NT> &a) {
#pragma unroll
    for (int r = 0; r < NT; ++r)
#pragma unroll
        for (int c = 0; c < NT; ++c) {
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
template <int NT>
__device__ __forceinline__ XT<NT> matvec(const AT<NT> &a, const XT<NT> &x) {
    XT<NT> d;
#pragma unroll
    for (int r = 0; r < NT; ++r) {
        f4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < NT; ++c) acc = mfma4v(a.a[r][c], x.t[c], acc);
        d.t[r] = acc;
    }
    return d;
}
// the same with the operands in LDS: la[(r * NT + c) * 64 + lane]
template <int NT>
__device__ __forceinline__ XT<NT> matvec_lds(const f4 *la, int lane, const XT<NT> &x) {
    XT<NT> d;
#pragma unroll
    for (int r = 0; r < NT; ++r) {
        f4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < NT; ++c) acc = mfma4v(la[(r * NT + c) * 64 + lane], x.t[c], acc);
        d.t[r] = acc;
    }
    return d;
}

// the lane's partial sums of the NT tile rows, added as a pairwise tree: (h0 + h1) [+ (h2 + h3)].  The order is part
// of the results' bits.
template <int N>
__device__ __forceinline__ float tree_sum(const float *h) {
    if constexpr (N == 1) return h[0];
    else return tree_sum<N / 2>(h) + tree_sum<N / 2>(h + N / 2);
}
template <int NT>
__device__ __forceinline__ float sum(const XT<NT> &x) {
    float h[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) h[t] = hsum(x.t[t]);
    return col_sum(tree_sum<NT>(h));
}
template <int NT>
__device__ __forceinline__ float sum_abs(const XT<NT> &x) {
    float h[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) h[t] = hsum_abs(x.t[t]);
    return col_sum(tree_sum<NT>(h));
}
// the lane's sum of the negative components (psi's flagged mass; the caller sums over the column)
template <int NT>
__device__ __forceinline__ float lane_sum_neg(const XT<NT> &x) {
    float h[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) h[t] = hsum_neg(x.t[t]);
    return tree_sum<NT>(h);
}
template <int NT>
__device__ __forceinline__ float dot(const XT<NT> &a, const XT<NT> &b) {
    float h[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) h[t] = hsum(a.t[t] * b.t[t]);
    return col_sum(tree_sum<NT>(h));
}

template <int NT>
__device__ __forceinline__ BT<NT> make_bounds(int g, int q, float eps) {
    BT<NT> b;
    const float inf = __builtin_inff();
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int s0 = 16 * t + 4 * g;
        b.t[t].lo.x = s0 + 0 < q ? eps : 0.f;  b.t[t].hi.x = s0 + 0 < q ? inf : 0.f;
        b.t[t].lo.y = s0 + 1 < q ? eps : 0.f;  b.t[t].hi.y = s0 + 1 < q ? inf : 0.f;
        b.t[t].lo.z = s0 + 2 < q ? eps : 0.f;  b.t[t].hi.z = s0 + 2 < q ? inf : 0.f;
        b.t[t].lo.w = s0 + 3 < q ? eps : 0.f;  b.t[t].hi.w = s0 + 3 < q ? inf : 0.f;
    }
    return b;
}
// emission rows s = 0 .. N-1 of this lane's chain: NT 16-byte loads per row (states 16 t + 4g ..); what lies past
// the row's q states is the next row (or, at the tensor's end, outside the descriptor: 0) and is zeroed by the clamp
// bounds
template <int NT, int N>
__device__ __forceinline__ void ld_rows(__amdgpu_buffer_rsrc_t r, int voff, int rowb, XT<NT> (&e)[N]) {
#pragma unroll
    for (int s = 0; s < N; ++s)
#pragma unroll
        for (int t = 0; t < NT; ++t)
            e[s].t[t] = __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(r, voff + s * rowb + 64 * t, 0, 0));
}
template <int NT>
__device__ __forceinline__ XT<NT> clamp(const XT<NT> &e, const BT<NT> &b) {
    XT<NT> r;
#pragma unroll
    for (int t = 0; t < NT; ++t) r.t[t] = clampE(e.t[t], b.t[t]);
    return r;
}
// a vector of the workspace ([chain][W]: prefix, suffix) or a checkpoint row
template <int NT>
__device__ __forceinline__ XT<NT> ld_vec(const float *v, int g) {
    XT<NT> r;
#pragma unroll
    for (int t = 0; t < NT; ++t) r.t[t] = *reinterpret_cast<const f4 *>(v + 16 * t + 4 * g);
    return r;
}
template <int NT>
__device__ __forceinline__ XT<NT> zero_vec() {
    XT<NT> r;
#pragma unroll
    for (int t = 0; t < NT; ++t) r.t[t] = (f4){0.f, 0.f, 0.f, 0.f};
    return r;
}

// a wave's 16 (sequence, chunk) pairs in the apply kernels: lane (g, n) works on pair n
struct ChainTile {
    long long wave, chain;
    bool valid, first;
    int len, voff, m;
    __amdgpu_buffer_rsrc_t rsE;
    const float *baseE;
};

__device__ __forceinline__ ChainTile make_chain_tile(const float *E, const Plan &p, long long wave, int g, int n) {
    const long long per_model = (long long)p.b * p.C;
    const long long wpm = (per_model + 15) / 16;
    ChainTile tl;
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
    tl.first = c == 0 && p.seq_start;        // (a later time slab's chunk 0 is an ordinary chunk: hmm_seqshard_mid_*)
    tl.len = tl.valid ? min(p.T, p.L - c * p.T) : 0;
    const long long row0 = seq0 * p.L + (long long)cc0 * p.T;
    const long long row = seq * p.L + (long long)c * p.T;
    tl.voff = (int)((row - row0) * p.q * (long long)sizeof(float)) + g * 16;
    const unsigned long long total = (unsigned long long)p.NB * p.L * p.q * sizeof(float);
    tl.baseE = E + row0 * p.q;
    tl.rsE = make_rsrc(tl.baseE, total - (unsigned long long)row0 * p.q * sizeof(float));
    return tl;
}

// output rows staged in wave-private LDS (per chain one contiguous run of rows, its image in HBM) and flushed as
// 16-byte pieces of contiguous memory — the OutStage of the 16-state kernels for rows of up to W states
template <int NT>
struct OutT {
    float *seg;                 // Rows<NT>::STAGE_SEG floats
    char *base;
    int q;
};
template <int NT>
__device__ __forceinline__ OutT<NT> make_out(float *seg, char *base, int q, int lane, int voff0, int len) {
    OutT<NT> o = {seg, base, q};
    int *tab = reinterpret_cast<int *>(seg + 16 * Rows<NT>::STAGE_STRIDE);
    if (lane < 16) { tab[lane] = voff0; tab[16 + lane] = len; }
    __builtin_amdgcn_wave_barrier();
    return o;
}
template <int NT>
__device__ __forceinline__ void stage(const OutT<NT> &o, int n, int g, int srow, const XT<NT> &v) {
    float *pr = o.seg + n * Rows<NT>::STAGE_STRIDE + srow * o.q;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int s0 = 16 * t + 4 * g;
        if (s0 + 0 < o.q) pr[s0 + 0] = v.t[t].x;
        if (s0 + 1 < o.q) pr[s0 + 1] = v.t[t].y;
        if (s0 + 2 < o.q) pr[s0 + 2] = v.t[t].z;
        if (s0 + 3 < o.q) pr[s0 + 3] = v.t[t].w;
    }
}
// rows row0 .. row0 + nrows - 1 of every chain (nrows is a multiple of 4: whole 16-byte pieces)
template <int NT>
__device__ __forceinline__ void flush(const OutT<NT> &o, int lane, int row0, int nrows) {
    const int *tab = reinterpret_cast<const int *>(o.seg + 16 * Rows<NT>::STAGE_STRIDE);
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
        const f4 v = *reinterpret_cast<const f4 *>(o.seg + c * Rows<NT>::STAGE_STRIDE + 4 * kk);
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

// DecodeMid's flush of the same rows: the chain table holds ROW offsets from `rowbase` (the wave's first row in the
// (k,b,L) outputs).  A lane takes one staged row of one chain (16 chains x nrows rows: up to 128 at NT = 2, 64 at
// NT = 4) and collapses it (collapse_row, hmm_midq.inc); a chain's ragged end and chains the wave does not own
// (len 0) are skipped through the table.  Every lane addresses its own byte, so a chunk may start at any byte offset.
// NT = 2 holds the row's 32 values in registers; NT = 4, at one wave per SIMD and up to 256 VGPRs, streams it in
// pieces of 16.
template <int NT>
__device__ __forceinline__ void decode_flush(const OutT<NT> &o, const DecodeMid &d, const float *wt, long long rowbase,
                                             int lane, int row0, int nrows) {
    const int *tab = reinterpret_cast<const int *>(o.seg + 16 * Rows<NT>::STAGE_STRIDE);
    const float inv = 1.0f / (float)nrows;
    __builtin_amdgcn_wave_barrier();
#pragma unroll 1
    for (int pc = lane; pc < 16 * nrows; pc += 64) {
        const int c = (int)(((float)pc + 0.5f) * inv);                    // pc / nrows, exact for these ranges
        const int r = pc - c * nrows;
        if (r >= tab[16 + c] - row0) continue;
        collapse_row<Rows<NT>::W, NT == 2 ? 32 : 16>(o.seg + c * Rows<NT>::STAGE_STRIDE + r * o.q, o.q, d, wt,
                                                     rowbase + tab[c] + row0 + r);
    }
    __builtin_amdgcn_wave_barrier();
}

// max(d, eps)'s clamp-born part, component-wise: where the clamp was active the whole eps is born there, elsewhere the
// carried clamp-born part df (forward_body's CERT / backward_body's CERT3 in hmm_engine.hip)
__device__ __forceinline__ f4 born4(f4 d, f4 df, float eps) {
    f4 r = {d.x > eps ? df.x : eps, d.y > eps ? df.y : eps, d.z > eps ? df.z : eps, d.w > eps ? df.w : eps};
    return r;
}

// ---- dense reduce: one wave per (sequence, chunk), the operator X (W x W) as NT x NT MFMA tiles — X[cb].t[r]: lane
// (g, n) holds rows 16 r + 4g .. + 3 of column 16 cb + n —, a step X <- diag(E_t) A^T X is NT^3 16x16x16 block
// products, columns rescaled by exact powers of two with an integer exponent per column, exactly as k_reduce does
// for 16 states.  2 q^3 flop per position: for 32 states at b = 1024 x L = 1e5 that alone is ~45 ms and no better
// than one wave per sequence (hmm_midq.inc, latency-bound whatever the batch), but the serial kernels take their
// ~66 ms for 16 sequences as for 1024, and this scales with the work.
template <int NT>
__global__ __launch_bounds__(256) void reduce_dense(const float *__restrict__ A, const float *__restrict__ E,
                                                    float *__restrict__ ops, int *__restrict__ exps,
                                                    int *__restrict__ riskv, const int *__restrict__ elig, Plan p,
                                                    float eps) {
    typedef Rows<NT> R;
    constexpr int W = R::W, PF = R::REDUCE_PF;
    const int lane = threadIdx.x & 63, g = lane >> 4, n = lane & 15;
    const int q = p.q;
    const long long stride = (long long)gridDim.x * 4;
    for (long long chain = (long long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
         chain < p.nchains; chain += stride) {
        const int seq = (int)(chain / p.C), c = (int)(chain - (long long)seq * p.C);
        const int m = seq / p.b;
        if (elig[m] != R::ID_DENSE) continue;
        const int t0 = c * p.T;
        const int len = min(p.T, p.L - t0);
        AT<NT> a;
        load_A<NT>(A + (size_t)m * q * q, q, g, n, true, a);
        const BT<NT> bd = make_bounds<NT>(g, q, eps);
        const float *base = E + ((size_t)seq * p.L + t0) * q;
        const __amdgpu_buffer_rsrc_t rs = make_rsrc(base, (unsigned long long)len * q * sizeof(float));
        const int rowb = q * (int)sizeof(float);
        int voff = g * 16;
        XT<NT> X[NT];                               // X[cb]: the NT row tiles of column block cb
#pragma unroll
        for (int cb = 0; cb < NT; ++cb)
#pragma unroll
            for (int r = 0; r < NT; ++r) {
                f4 v;
                v.x = 16 * r + 4 * g + 0 == 16 * cb + n ? 1.f : 0.f;
                v.y = 16 * r + 4 * g + 1 == 16 * cb + n ? 1.f : 0.f;
                v.z = 16 * r + 4 * g + 2 == 16 * cb + n ? 1.f : 0.f;
                v.w = 16 * r + 4 * g + 3 == 16 * cb + n ? 1.f : 0.f;
                X[cb].t[r] = v;
            }
        int ex[NT] = {};                            // column 16 cb + n holds X[:, .] * 2^-ex[cb]
        // risk: EVERY column lost more than 2^-45 in ONE step — an observation that everything survives at the emission floor
        // only —, or a column's sum went below 2^-100 (the denormal range: reduce_sparse_wave's `risk`).  Such sequences
        // go to the serial kernels (the mark: riskv[chain], read by k_scan_select).  The exponent is clamped at -100 so
        // that the factor stays finite for a column in the denormal range.
        bool risk = false;
        auto rescale = [&]() {
            bool kept = false;                      // some column lost less than 2^-45 in this step
#pragma unroll
            for (int cb = 0; cb < NT; ++cb) {
                const float sden = sum<NT>(X[cb]);
                risk = risk || (16 * cb + n < q && sden < 0x1p-100f);
                const int xe = max(__builtin_amdgcn_frexp_expf(sden), -100);
                kept = kept || (16 * cb + n < q && !(xe < -45));
                const float sc = __builtin_amdgcn_ldexpf(1.0f, -xe);
#pragma unroll
                for (int r = 0; r < NT; ++r) X[cb].t[r] = X[cb].t[r] * sc;
                ex[cb] += xe;
            }
            risk = risk || __builtin_amdgcn_ballot_w64(kept) == 0ull;      // EVERY column, whatever the start state
        };
        int t = 0;
        if (c == 0 && p.seq_start) {                // first observation of the sequence: no transition
            XT<NT> e0[1];
            ld_rows<NT, 1>(rs, voff, rowb, e0);
            const XT<NT> ec = clamp<NT>(e0[0], bd);
#pragma unroll
            for (int cb = 0; cb < NT; ++cb)
#pragma unroll
                for (int r = 0; r < NT; ++r) X[cb].t[r] = X[cb].t[r] * ec.t[r];
            rescale();
            voff += rowb;
            t = 1;
        }
        XT<NT> en[PF];
        ld_rows<NT, PF>(rs, voff, rowb, en);
        for (; t < len; t += PF) {
            XT<NT> ec[PF];
#pragma unroll
            for (int u = 0; u < PF; ++u) ec[u] = clamp<NT>(en[u], bd);
            voff += PF * rowb;
            ld_rows<NT, PF>(rs, voff, rowb, en);    // (past the chunk: outside the descriptor, zeros)
#pragma unroll
            for (int u = 0; u < PF; ++u) {
                if (t + u < len) {                  // wave-uniform
#pragma unroll
                    for (int cb = 0; cb < NT; ++cb) {
                        const XT<NT> d = matvec<NT>(a, X[cb]);
#pragma unroll
                        for (int r = 0; r < NT; ++r) X[cb].t[r] = d.t[r] * ec[u].t[r];
                    }
                    rescale();
                }
            }
        }
        float *o = ops + (size_t)chain * W * W;
#pragma unroll
        for (int cb = 0; cb < NT; ++cb) {
#pragma unroll
            for (int r = 0; r < NT; ++r) {
                o[(16 * r + 4 * g + 0) * W + 16 * cb + n] = X[cb].t[r].x;
                o[(16 * r + 4 * g + 1) * W + 16 * cb + n] = X[cb].t[r].y;
                o[(16 * r + 4 * g + 2) * W + 16 * cb + n] = X[cb].t[r].z;
                o[(16 * r + 4 * g + 3) * W + 16 * cb + n] = X[cb].t[r].w;
            }
            if (g == 0) exps[(size_t)chain * W + 16 * cb + n] = 16 * cb + n < q ? ex[cb] : 0;
        }
        const bool mark = __builtin_amdgcn_ballot_w64(risk) != 0ull;
        if (lane == 0) riskv[chain] = mark ? 1 : 0;
    }
}

// ---- scan over W x W chunk operators: ops[chain][i][k] (i = state at the chunk's last step, k = state just before
// the chunk, column k scaled by 2^-exps[k]).  One 128-thread block per sequence, wave 0 the forward prefix chain,
// wave 1 the backward suffix chain; lane = state (rows of 32: lanes 32..63 carry zeros; all lanes stay active: the
// wave-wide sums and maxima are DPP / permlane reductions).
__device__ __forceinline__ float wave_sum(float v) { return col_sum(row_sum_f(v)); }
__device__ __forceinline__ int wave_max(int v) { return col_max_i(row_max_i(v)); }

// a hop's common exponent: the vector's components x in the scale of their operator columns (2^-xec), brought to
// the largest one (*emax) by an exact power of two, at most 2^-300
__device__ __forceinline__ float hop_align(float x, int xec, int *emax) {
    const int we = (x > 0.f) ? __builtin_amdgcn_frexp_expf(x) + xec : -(1 << 28);
    *emax = wave_max(we);
    int sh = xec - *emax;
    sh = sh < -300 ? -300 : sh;
    return __builtin_amdgcn_ldexpf(x, sh);
}

template <int NT>
__global__ __launch_bounds__(128) void scan(const float *__restrict__ pi, const float *__restrict__ ops,
                                           const int *__restrict__ exps, float *__restrict__ prefix,
                                           double *__restrict__ llpre, float *__restrict__ suffix,
                                           double *__restrict__ lsuf, double *__restrict__ loglik,
                                           const int *__restrict__ elig, Plan p, float eps,
                                           const float *__restrict__ entry_pre, const double *__restrict__ entry_ll,
                                           const float *__restrict__ entry_suf, const double *__restrict__ entry_ls) {
    // entry_pre / entry_ll / entry_suf / entry_ls (null: the start distribution and ones): the vectors entering a time
    // slab from the slabs before / after it ([seq][W], hmm_seqshard_mid_*), as k_scan takes them for 16 states
    constexpr int W = Rows<NT>::W;
    constexpr bool PRE = Rows<NT>::SCAN_PREFETCH;
    const int seq = blockIdx.x;
    const int lane = threadIdx.x & 63;
    const int dir = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int q = p.q, C = p.C;
    const int m = seq / p.b;
    if (elig[m] == 0) return;
    const size_t chain0 = (size_t)seq * C;
    const bool act = lane < q;
    const int n = lane & (W - 1);
    if (dir == 0) {
        // (a given entry vector is taken as it is: the clamp belongs to pi only)
        const float praw = act ? (entry_pre ? entry_pre[(size_t)seq * W + lane] : pi[(size_t)m * q + lane]) : 0.f;
        float a = entry_pre ? praw : (act ? fmaxf(praw, eps) : 0.f);
        double ll = entry_ll ? entry_ll[seq] : 0.0;
        if (lane < W) prefix[chain0 * W + lane] = praw;
        if (lane == 0) llpre[chain0] = 0.0;
        f4 rw[W / 4];                                        // row n of operator c
        int xe = 0;
        auto fetch = [&](int c) {
            const f4 *row = reinterpret_cast<const f4 *>(ops + (chain0 + c) * W * W + n * W);
#pragma unroll
            for (int u = 0; u < W / 4; ++u) rw[u] = row[u];
            xe = exps[(chain0 + c) * W + n];
        };
        if (PRE) fetch(0);
        for (int c = 0; c < C; ++c) {
            if (!PRE) fetch(c);
            f4 cur[W / 4];
#pragma unroll
            for (int u = 0; u < W / 4; ++u) cur[u] = rw[u];
            const int xec = xe;
            if (PRE && c + 1 < C) fetch(c + 1);
            int emax;
            const float w = hop_align(a, xec, &emax);
            float acc = 0.f;
#pragma unroll
            for (int u = 0; u < W / 4; ++u) {
                acc = fmaf(cur[u].x, lane_bcast(w, 4 * u + 0), acc);
                acc = fmaf(cur[u].y, lane_bcast(w, 4 * u + 1), acc);
                acc = fmaf(cur[u].z, lane_bcast(w, 4 * u + 2), acc);
                acc = fmaf(cur[u].w, lane_bcast(w, 4 * u + 3), acc);
            }
            acc = act ? acc : 0.f;
            const float S = wave_sum(acc);
            a = acc / S;
            ll += (double)__logf(S) + (double)emax * LN2;
            if (c + 1 < C) {
                if (lane < W) prefix[(chain0 + c + 1) * W + lane] = a;
                if (lane == 0) llpre[chain0 + c + 1] = ll;
            }
        }
        if (lane == 0) loglik[seq] = ll;
    } else {
        float v = act ? (entry_suf ? entry_suf[(size_t)seq * W + lane] : 1.f) : 0.f;
        double lb = entry_ls ? entry_ls[seq] : 0.0;
        float col[PRE ? W : 1];                              // PRE: column n of the next operator
        int xe = 0;
        auto fetch = [&](int c) {
            const float *X = ops + (chain0 + c) * W * W;
            if constexpr (PRE) {
#pragma unroll
                for (int j = 0; j < W; ++j) col[j] = X[j * W + n];
            }
            xe = exps[(chain0 + c) * W + n];
        };
        if (PRE && C > 1) fetch(C - 1);
        for (int c = C - 1; c >= 0; --c) {
            if (lane < W) suffix[(chain0 + c) * W + lane] = v;
            if (lane == 0) lsuf[chain0 + c] = lb;
            if (c == 0) break;
            if (!PRE) fetch(c);
            const int xec = xe;
            float u = 0.f;
            if constexpr (PRE) {
                float cc[W];
#pragma unroll
                for (int j = 0; j < W; ++j) cc[j] = col[j];
                if (c - 1 > 0) fetch(c - 1);
#pragma unroll
                for (int j = 0; j < W; ++j) u = fmaf(cc[j], lane_bcast(v, j), u);
            } else {
                const float *X = ops + (chain0 + c) * W * W;
#pragma unroll 16
                for (int j = 0; j < W; ++j) u = fmaf(X[j * W + n], lane_bcast(v, j), u);
            }
            u = act ? u : 0.f;
            int emax;
            v = hop_align(u, xec, &emax);
            lb += (double)emax * LN2;
        }
    }
}

// ---- compose: k_scan_compose at width W.  One wave per (sequence, group): X <- Op_c X over the group's operators
// (chunks c0 .. c1 - 1 of ops[seq][p.C]), X the identity at the start and held as reduce_dense holds it (X[cb].t[r]:
// lane (g, n) has rows 16 r + 4g .. + 3 of column 16 cb + n, the column scaled by 2^-ex[cb]).  The hops carry no
// clamp, so operators compose exactly up to rounding; the sequence-sharded posterior (hmm_seqshard_mid_*) forms a time
// slab's operator this way, in two levels for long slabs.  Per hop and column: the rows are aligned to a common
// exponent (their own plus the exponent of the operator column they meet; the shift clamped at -300), multiplied, and
// the column sum brought back into [0.5, 1) by an exact power of two.  A column without a positive entry stays zero
// (emax = 0), and the factor stays finite for a sum in the denormal range (the exponent clamped at -100, as in
// reduce_dense).  Rows, columns and exponents from q on are written as 0.  The next operator is in flight during a hop.
template <int NT>
__global__ __launch_bounds__(256) void compose(const float *__restrict__ ops, const int *__restrict__ exps,
                                               float *__restrict__ gops, int *__restrict__ gexps, Plan p) {
    constexpr int W = Rows<NT>::W;
    const long long wv = (long long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (wv >= (long long)p.NB * p.G) return;
    const int lane = threadIdx.x & 63, g = lane >> 4, n = lane & 15;
    const int q = p.q;
    const int seq = (int)(wv / p.G), grp = (int)(wv - (long long)seq * p.G);
    const int c0 = grp * p.gsize, c1 = min(p.C, c0 + p.gsize);
    XT<NT> X[NT];
#pragma unroll
    for (int cb = 0; cb < NT; ++cb)
#pragma unroll
        for (int r = 0; r < NT; ++r) {
            const int col = 16 * cb + n, row = 16 * r + 4 * g;
            const bool on = col < q;
            X[cb].t[r] = (f4){on && row + 0 == col ? 1.f : 0.f, on && row + 1 == col ? 1.f : 0.f,
                              on && row + 2 == col ? 1.f : 0.f, on && row + 3 == col ? 1.f : 0.f};
        }
    int ex[NT] = {};
    const size_t chb = (size_t)seq * p.C;
    // A-operand: lane (g, i = n) supplies Op[16 r + i][16 c + 4g + kk]; en[r]: exponents of the contraction rows
    AT<NT> an;
    i4 en[NT];
    auto fetch = [&](int c) {
        const float *op = ops + (chb + c) * W * W;
        const int *oe = exps + (chb + c) * W;
#pragma unroll
        for (int r = 0; r < NT; ++r) {
#pragma unroll
            for (int cc = 0; cc < NT; ++cc) an.a[r][cc] = *reinterpret_cast<const f4 *>(op + (16 * r + n) * W + 16 * cc + 4 * g);
            const i4 e = *reinterpret_cast<const i4 *>(oe + 16 * r + 4 * g);
            const int s0 = 16 * r + 4 * g;                   // (the pad lanes carry no exponent: the sparse reduce's mark)
            en[r] = (i4){s0 + 0 < q ? e.x : 0, s0 + 1 < q ? e.y : 0, s0 + 2 < q ? e.z : 0, s0 + 3 < q ? e.w : 0};
        }
    };
    fetch(c0);
    for (int c = c0; c < c1; ++c) {
        const AT<NT> a = an;
        i4 e[NT];
#pragma unroll
        for (int r = 0; r < NT; ++r) e[r] = en[r];
        if (c + 1 < c1) fetch(c + 1);
#pragma unroll
        for (int cb = 0; cb < NT; ++cb) {
            int we = -(1 << 28);
#pragma unroll
            for (int r = 0; r < NT; ++r) {
                const f4 x = X[cb].t[r];
                we = x.x > 0.f ? max(we, __builtin_amdgcn_frexp_expf(x.x) + e[r].x) : we;
                we = x.y > 0.f ? max(we, __builtin_amdgcn_frexp_expf(x.y) + e[r].y) : we;
                we = x.z > 0.f ? max(we, __builtin_amdgcn_frexp_expf(x.z) + e[r].z) : we;
                we = x.w > 0.f ? max(we, __builtin_amdgcn_frexp_expf(x.w) + e[r].w) : we;
            }
            int emax = col_max_i(we);
            emax = emax == -(1 << 28) ? 0 : emax;
            XT<NT> w;
#pragma unroll
            for (int r = 0; r < NT; ++r) {
                const f4 x = X[cb].t[r];
                w.t[r] = (f4){__builtin_amdgcn_ldexpf(x.x, max(e[r].x - emax, -300)),
                              __builtin_amdgcn_ldexpf(x.y, max(e[r].y - emax, -300)),
                              __builtin_amdgcn_ldexpf(x.z, max(e[r].z - emax, -300)),
                              __builtin_amdgcn_ldexpf(x.w, max(e[r].w - emax, -300))};
            }
            const XT<NT> d = matvec<NT>(a, w);
            // bring the column sum back into [0.5, 1): exact power of two
            const int xe = max(__builtin_amdgcn_frexp_expf(sum<NT>(d)), -100);
            const float sc = __builtin_amdgcn_ldexpf(1.0f, -xe);
#pragma unroll
            for (int r = 0; r < NT; ++r) X[cb].t[r] = d.t[r] * sc;
            ex[cb] += emax + xe;
        }
    }
    float *o = gops + (size_t)wv * W * W;
#pragma unroll
    for (int cb = 0; cb < NT; ++cb) {
        const int col = 16 * cb + n;
#pragma unroll
        for (int r = 0; r < NT; ++r) {
            const int row = 16 * r + 4 * g;
            o[(row + 0) * W + col] = col < q && row + 0 < q ? X[cb].t[r].x : 0.f;
            o[(row + 1) * W + col] = col < q && row + 1 < q ? X[cb].t[r].y : 0.f;
            o[(row + 2) * W + col] = col < q && row + 2 < q ? X[cb].t[r].z : 0.f;
            o[(row + 3) * W + col] = col < q && row + 3 < q ? X[cb].t[r].w : 0.f;
        }
        if (g == 0) gexps[(size_t)wv * W + col] = col < q ? ex[cb] : 0;
    }
}

// entry vectors of slab r out of the global hops' per-slab vectors [seq][R] (k_seqshard_pick at width W)
__global__ __launch_bounds__(256) void k_mid_pick(const float *__restrict__ gpre, const double *__restrict__ gll,
                                                  const float *__restrict__ gsuf, const double *__restrict__ gls,
                                                  float *__restrict__ pre, double *__restrict__ ll,
                                                  float *__restrict__ suf, double *__restrict__ ls, int NB, int R, int r,
                                                  int W) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)NB * W) return;
    const long long seq = i / W;
    const int n = (int)(i - seq * W);
    pre[i] = gpre[((size_t)seq * R + r) * W + n];
    suf[i] = gsuf[((size_t)seq * R + r) * W + n];
    if (n == 0) { ll[seq] = gll[(size_t)seq * R + r]; ls[seq] = gls[(size_t)seq * R + r]; }
}

// phi_out[seq] = the time slab's share of the sequence's clamp-born posterior mass: psi of backward<NT> summed over
// the slab's chunks, a whole 1 for every chain a reduce marked (where the marks live: k_scan_select); +inf when the
// model's support is not primitive (prim[m] == 0: the model check under HMM_EXACT_AUTO)
__global__ __launch_bounds__(256) void k_mid_phi(const float *__restrict__ psi, const int *__restrict__ elig,
                                                 const int *__restrict__ prim, const int *__restrict__ exps,
                                                 const int *__restrict__ risk, float *__restrict__ phi_out, Plan p,
                                                 int W) {
    const int seq = blockIdx.x * 256 + threadIdx.x;
    if (seq >= p.NB) return;
    const int m = seq / p.b;
    const bool dense = elig_dense(elig[m]);
    float s = 0.f;
    for (int c = 0; c < p.C; ++c) {
        const size_t chain = (size_t)seq * p.C + c;
        s += psi[chain];
        if (dense ? risk[chain] != 0 : exps[chain * W + W - 1] != 0) s += 1.f;
    }
    phi_out[seq] = prim[m] == 0 ? __builtin_inff() : s;
}

// ---- apply, forward.  LOGA = false, CERT = false: alpha_hat entering every BLK-step block -> ckpt
// ([wave][block][chain][W]), nothing else;
// LOGA = true: log alpha_t = log alpha_hat_t + sum_{s<=t} log c_s -> out (hmm_forward with log alpha)
// CERT (hmm_forward, which has no backward pass to sum psi in): forward_body's CERT in hmm_engine.hip — the part of
//   alpha_hat born from the forward cell's clamps inside this chunk is carried along (Fv) and weighed at the chunk's
//   last position with the chunk scan's suffix vector there -> phi[chain]; with LOGA also the clamp-born share of
//   alpha_hat itself at the chunk's end, and what it becomes under the next observation (shnext).  CERT without LOGA
//   (the log-likelihood alone) writes nothing but phi.
template <int NT, bool LOGA, bool CERT>
__global__ __launch_bounds__(256) void forward(const float *__restrict__ A, const float *__restrict__ E,
                                               const float *__restrict__ prefix, const double *__restrict__ llpre,
                                               float *__restrict__ ckpt, float *__restrict__ out,
                                               const int *__restrict__ elig, Plan p, float eps, long long nwaves,
                                               const float *__restrict__ suffix, float *__restrict__ phi) {
    typedef Rows<NT> R;
    constexpr int W = R::W, BLK = R::BLK;
    constexpr bool CKPT = !LOGA && !CERT;
    const long long wave = (long long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (wave >= nwaves) return;
    const int lane = threadIdx.x & 63, g = lane >> 4, n = lane & 15;
    const int q = p.q;
    const ChainTile tl = make_chain_tile(E, p, wave, g, n);
    if (elig[tl.m] == 0) return;
    AT<NT> a;
    load_A<NT>(A + (size_t)tl.m * q * q, q, g, n, true, a);
    const BT<NT> bd = make_bounds<NT>(g, q, eps);
    const int rowb = q * (int)sizeof(float);
    XT<NT> X = ld_vec<NT>(prefix + (size_t)tl.chain * W, g);
    XT<NT> Fv = zero_vec<NT>(), Xc = X, Fc = zero_vec<NT>();   // CERT: clamp-born part of X; both at the chain's last step
    float *ck = CKPT ? ckpt + (((size_t)wave * p.nsub) * 16 + n) * W + 4 * g : nullptr;
    __shared__ __attribute__((aligned(16))) float ostage[LOGA ? 4 * R::STAGE_SEG : 4];
    OutT<NT> os = {};
    if (LOGA)
        os = make_out<NT>(ostage + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) * R::STAGE_SEG,
                          reinterpret_cast<char *>(out + (tl.baseE - E)), q, lane, tl.voff - g * 16, tl.len);
    double llb = LOGA ? llpre[tl.chain] : 0.0;
    constexpr int GB = R::STAGE_ROWS / BLK;                    // blocks per flush group
    int voff = tl.voff;
    XT<NT> en[BLK];
    ld_rows<NT, BLK>(tl.rsE, voff, rowb, en);
    for (int j = 0; j < p.nsub; ++j) {
        if (CKPT && tl.valid && j * BLK < tl.len) {
#pragma unroll
            for (int t = 0; t < NT; ++t) *reinterpret_cast<f4 *>(ck + (size_t)j * 16 * W + 16 * t) = X.t[t];
        }
        XT<NT> e[BLK];
#pragma unroll
        for (int s = 0; s < BLK; ++s) e[s] = en[s];
        if (j + 1 < p.nsub) ld_rows<NT, BLK>(tl.rsE, voff + BLK * rowb, rowb, en);
        float lacc = 0.f;
#pragma unroll
        for (int s = 0; s < BLK; ++s) {
            // one exact forward cell step: X <- normalise(max(E, eps) * max(X A, eps))
            const bool init = tl.first && j == 0 && s == 0;
            const XT<NT> ec = clamp<NT>(e[s], bd);
            const XT<NT> d = matvec<NT>(a, X);
            XT<NT> sf;
#pragma unroll
            for (int t = 0; t < NT; ++t) sf.t[t] = fmax4(sel4(init, X.t[t], d.t[t]), eps) * ec.t[t];
            const float S = sum<NT>(sf);
            const float inv = __builtin_amdgcn_rcpf(S);
            if (CERT) {
                const XT<NT> df = matvec<NT>(a, Fv);
                const bool last = j * BLK + s + 1 == tl.len;
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    // (pi's own clamp: the scan has it)
                    Fv.t[t] = sel4(init, Fv.t[t], born4(d.t[t], df.t[t], eps)) * ec.t[t] * inv;
                    X.t[t] = sf.t[t] * inv;
                    Xc.t[t] = sel4(last, X.t[t], Xc.t[t]);
                    Fc.t[t] = sel4(last, Fv.t[t], Fc.t[t]);
                }
            } else {
#pragma unroll
                for (int t = 0; t < NT; ++t) X.t[t] = sf.t[t] * inv;
            }
            if (LOGA) {
                lacc += (j * BLK + s < tl.len) ? __logf(S) : 0.f;
                const float base = (float)(llb + (double)lacc);
                XT<NT> la;
#pragma unroll
                for (int t = 0; t < NT; ++t) la.t[t] = log4(X.t[t]) + base;
                stage<NT>(os, n, g, (j % GB) * BLK + s, la);
            }
        }
        if (LOGA) {
            llb += (double)lacc;
            if ((j + 1) % GB == 0 || j + 1 == p.nsub) flush<NT>(os, lane, (j / GB) * R::STAGE_ROWS, (j % GB + 1) * BLK);
        }
        voff += BLK * rowb;
    }
    if (CERT) {
        const XT<NT> sv = ld_vec<NT>(suffix + (size_t)tl.chain * W, g);
        float c = dot<NT>(Fc, sv) * __builtin_amdgcn_rcpf(dot<NT>(Xc, sv));
        if (LOGA) {
            // the clamp-born share of alpha_hat where the chunk hands over, and what it becomes one step on under the
            // next observation (the first row of the chunk after, whose kernel starts from the floor-free prefix vector)
            XT<NT> en1 = zero_vec<NT>();
            const bool more = tl.valid && tl.chain % p.C != p.C - 1;            // (not the sequence's last chunk)
            if (more) {
                XT<NT> r1[1];
                ld_rows<NT, 1>(tl.rsE, tl.voff + tl.len * rowb, rowb, r1);
                en1 = clamp<NT>(r1[0], bd);
            }
            XT<NT> dx = matvec<NT>(a, Xc);
            const XT<NT> df = matvec<NT>(a, Fc);
#pragma unroll
            for (int t = 0; t < NT; ++t) dx.t[t] = fmax4(dx.t[t], eps);
            const float dn = dot<NT>(en1, dx);
            const float shnext = (more && dn > 0.f) ? dot<NT>(en1, df) * __builtin_amdgcn_rcpf(dn) : 0.f;
            c = fmaxf(fmaxf(c, sum<NT>(Fc)), shnext);
        }
        if (tl.valid && g == 0) phi[tl.chain] = c;
    }
}

// ---- apply, backward: posteriors.  MODE 0: gamma, 1: log gamma, 2: log gamma + loglik, 3: log beta (no forward part).
// phi: psi, the posterior mass of clamp-born paths (backward_body in hmm_engine.hip), per chain.
// CERT3 (MODE 3, hmm_backward): backward_body's CERT3 — the part of R born from the reverse cell's clamps inside this
//   chunk is carried along (Gv) and weighed at the chunk's first position with alpha_hat there, one forward step from
//   the chunk scan's prefix vector (a uniform start); also the clamp-born share of R where the chunk hands over to the
//   one before, and what it becomes under that chunk's last observation -> phi[chain]
// DEC: the output policy (MODE 0), the kernel's last argument.  NoDecode (an empty argument) flushes the staged gamma
// rows (flush<NT>); DecodeMid (hmm_posterior_decode_mid; no `out`) collapses them (decode_flush<NT>) with the block's
// weight table in LDS — everything up to the staged row is shared.
template <int NT, int MODE, bool CERT3, class DEC = NoDecode>
__global__ __launch_bounds__(256) void backward(const float *__restrict__ A, const float *__restrict__ E,
                                                const float *__restrict__ ckpt, const float *__restrict__ suffix,
                                                const double *__restrict__ lsuf, const double *__restrict__ loglik,
                                                float *__restrict__ out, float *__restrict__ phi,
                                                const int *__restrict__ elig, Plan p, float eps, long long nwaves,
                                                const float *__restrict__ prefix, const DEC dec) {
    static_assert(!CERT3 || MODE == 3, "CERT3 is the log beta certificate");
    static_assert(!DEC::on || MODE == 0, "labels are decoded from the probability output");
    const float *wt = nullptr;
    if constexpr (DEC::on) {                                 // (the whole block, before any wave leaves)
        __shared__ __attribute__((aligned(16))) float wts[MID_WT_FLOATS];
        mid_weights(dec, wts);
        wt = wts;
    }
    typedef Rows<NT> R;
    constexpr int W = R::W, BLK = R::BLK;
    const long long wave = (long long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (wave >= nwaves) return;
    const int lane = threadIdx.x & 63, g = lane >> 4, n = lane & 15;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int q = p.q;
    const ChainTile tl = make_chain_tile(E, p, wave, g, n);
    if (elig[tl.m] == 0) return;
    const float *Am = A + (size_t)tl.m * q * q;
    AT<NT> af, ab;                                           // forward (A^T) and backward (A) operands
    load_A<NT>(Am, q, g, n, false, ab);
    const f4 *la = nullptr;
    if constexpr (R::BWD_A_LDS) {
        __shared__ __attribute__((aligned(16))) f4 abl[4 * NT * NT * 64];   // [wave][(r, c)][lane]
        f4 *lw = abl + w * NT * NT * 64;
#pragma unroll
        for (int r = 0; r < NT; ++r)
#pragma unroll
            for (int c = 0; c < NT; ++c) lw[(r * NT + c) * 64 + lane] = ab.a[r][c];
        __builtin_amdgcn_wave_barrier();
        la = lw;
    }
    auto matvec_b = [&](const XT<NT> &x) {
        if constexpr (R::BWD_A_LDS) return matvec_lds<NT>(la, lane, x);
        else return matvec<NT>(ab, x);
    };
    if (MODE != 3 || (CERT3 && !R::BWD_A_LDS)) load_A<NT>(Am, q, g, n, true, af);
    const BT<NT> bd = make_bounds<NT>(g, q, eps);
    const int rowb = q * (int)sizeof(float);
    __shared__ __attribute__((aligned(16))) float ostage[4 * R::STAGE_SEG];
    // (DecodeMid: the chain table in rows, not bytes, and the wave's first row in place of a base pointer)
    const OutT<NT> os = DEC::on ? make_out<NT>(ostage + w * R::STAGE_SEG, nullptr, q, lane, (tl.voff - g * 16) / rowb, tl.len)
                                : make_out<NT>(ostage + w * R::STAGE_SEG, reinterpret_cast<char *>(out + (tl.baseE - E)), q,
                                               lane, tl.voff - g * 16, tl.len);
    const long long rowbase = DEC::on ? (long long)(tl.baseE - E) / q : 0;

    XT<NT> Rv = ld_vec<NT>(suffix + (size_t)tl.chain * W, g);
    float llf = 0.f;
    if (MODE == 2) llf = (float)loglik[tl.chain / p.C];
    double lbb = MODE == 3 ? lsuf[tl.chain] : 0.0;
    const float *ck = MODE == 3 ? nullptr : ckpt + (((size_t)wave * p.nsub) * 16 + n) * W + 4 * g;
    float phiacc = 0.f;
    const f4 zero4 = {0.f, 0.f, 0.f, 0.f};
    // CERT3: clamp-born part of R; R, Gv, E at the first position
    XT<NT> Gv = zero_vec<NT>(), Rc = Rv, Gc = zero_vec<NT>(), ec0 = zero_vec<NT>();

    XT<NT> en[BLK], Xn = zero_vec<NT>();
    auto fetch = [&](int jb) {                               // block jb's emission rows, and the alpha_hat entering it
        ld_rows<NT, BLK>(tl.rsE, tl.voff + jb * BLK * rowb, rowb, en);
        if (MODE != 3) {
#pragma unroll
            for (int t = 0; t < NT; ++t)
                Xn.t[t] = (tl.valid && jb * BLK < tl.len) ? *reinterpret_cast<const f4 *>(ck + (size_t)jb * 16 * W + 16 * t) : zero4;
        }
    };
    if (R::BWD_PREFETCH) fetch(p.nsub - 1);
    constexpr int GB = R::STAGE_ROWS / BLK;                    // blocks per flush group
    for (int j = p.nsub - 1; j >= 0; --j) {
        const int srow = (j % GB) * BLK;
        if (!R::BWD_PREFETCH) fetch(j);
        XT<NT> e[BLK];
#pragma unroll
        for (int s = 0; s < BLK; ++s) e[s] = clamp<NT>(en[s], bd);
        XT<NT> X = Xn;
        if (R::BWD_PREFETCH && j > 0) fetch(j - 1);
        // (alpha_hat and R carry "the clamp of this component's prediction was active" in their sign bits: psi,
        // see backward_body in hmm_engine.hip)
        XT<NT> fa[BLK];
        if (MODE != 3) {
#pragma unroll
            for (int s = 0; s < BLK; ++s) {
                const bool init = tl.first && j == 0 && s == 0;
                const XT<NT> d = matvec<NT>(af, X);
                XT<NT> sf;
#pragma unroll
                for (int t = 0; t < NT; ++t)
                    sf.t[t] = sel4(init, fmax4(X.t[t], eps), clamp_flag4(d.t[t], eps)) * e[s].t[t];
                const float inv = __builtin_amdgcn_rcpf(sum_abs<NT>(sf));
#pragma unroll
                for (int t = 0; t < NT; ++t) { fa[s].t[t] = sf.t[t] * inv; X.t[t] = abs4(fa[s].t[t]); }
            }
        }
        float lacc = 0.f;
#pragma unroll
        for (int s = BLK - 1; s >= 0; --s) {
            const bool act = j * BLK + s < tl.len;
            XT<NT> gm;
            if (MODE == 3) {
                const float base = (float)(lbb + (double)lacc);
#pragma unroll
                for (int t = 0; t < NT; ++t) gm.t[t] = log4(Rv.t[t]) + base;
            } else {
#pragma unroll
                for (int t = 0; t < NT; ++t) gm.t[t] = fa[s].t[t] * Rv.t[t];       // negative: exactly one clamp was active
                const float Sg = sum_abs<NT>(gm);
                const float ig = __builtin_amdgcn_rcpf(Sg);
                phiacc = fmaf(lane_sum_neg<NT>(gm), act ? ig : 0.f, phiacc);
                if (MODE == 0) {
#pragma unroll
                    for (int t = 0; t < NT; ++t) gm.t[t] = mul_abs4(gm.t[t], f4{ig, ig, ig, ig});
                } else {
                    const float lg = __logf(Sg) - llf;
#pragma unroll
                    for (int t = 0; t < NT; ++t) gm.t[t] = log4(abs4(gm.t[t])) - lg;
                }
            }
            stage<NT>(os, n, g, srow + s, gm);
            if (CERT3 && s == 0) { Rc = Rv; Gc = Gv; ec0 = e[0]; }      // (the last block executed is the chunk's first)
            XT<NT> sf;
#pragma unroll
            for (int t = 0; t < NT; ++t) sf.t[t] = MODE == 3 ? e[s].t[t] * Rv.t[t] : mul_abs4(Rv.t[t], e[s].t[t]);
            const float Sb = sum<NT>(sf);
            if (MODE == 3) lacc += act ? __logf(Sb) : 0.f;
            const float ib = __builtin_amdgcn_rcpf(Sb);
#pragma unroll
            for (int t = 0; t < NT; ++t) sf.t[t] = sf.t[t] * ib;
            const XT<NT> d = matvec_b(sf);
            if (CERT3) {
                XT<NT> gs;
#pragma unroll
                for (int t = 0; t < NT; ++t) gs.t[t] = e[s].t[t] * Gv.t[t] * ib;
                const XT<NT> ug = matvec_b(gs);
#pragma unroll
                for (int t = 0; t < NT; ++t) Gv.t[t] = sel4(act, born4(d.t[t], ug.t[t], eps), Gv.t[t]);
            }
#pragma unroll
            for (int t = 0; t < NT; ++t)
                Rv.t[t] = sel4(act, MODE == 3 ? fmax4(d.t[t], eps) : clamp_flag4(d.t[t], eps), Rv.t[t]);
        }
        if (MODE == 3) lbb += (double)lacc;
        if (j % GB == 0) {
            const int top = p.nsub - j;
            if constexpr (DEC::on) decode_flush<NT>(os, dec, wt, rowbase, lane, j * BLK, (top < GB ? top : GB) * BLK);
            else flush<NT>(os, lane, j * BLK, (top < GB ? top : GB) * BLK);
        }
    }
    if (MODE != 3) {
        // The handover.  Rv is now R at the last position of the chunk before, with the flags of the clamp that made it;
        // the gamma that weighs them belongs to that chunk, whose kernel starts from the chunk scan's suffix vector: the
        // same direction without the clamp.  It is weighed here, with alpha_hat at that position (the vector entering
        // this chunk: block 0's checkpoint), and charged to this chunk (k_exact_select in hmm_engine.hip does the same
        // for up to 16 states).
        const bool hand = tl.valid && !tl.first;
        XT<NT> gm;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const f4 x0 = hand ? *reinterpret_cast<const f4 *>(ck + 16 * t) : zero4;
            gm.t[t] = abs4(x0) * Rv.t[t];
        }
        const float ig = __builtin_amdgcn_rcpf(sum_abs<NT>(gm));
        phiacc = fmaf(lane_sum_neg<NT>(gm), hand ? ig : 0.f, phiacc);
    }
    phiacc = col_sum(phiacc);
    if (MODE != 3 && g == 0 && tl.valid) phi[tl.chain] = phiacc;
    if (CERT3) {
        // alpha_hat at the chunk's first position, up to scale: one forward step from the vector entering the chunk
        if (R::BWD_A_LDS) load_A<NT>(Am, q, g, n, true, af);
        const XT<NT> P = ld_vec<NT>(prefix + (size_t)tl.chain * W, g);
        const XT<NT> dp = matvec<NT>(af, P);
        XT<NT> a0;
#pragma unroll
        for (int t = 0; t < NT; ++t) a0.t[t] = fmax4(sel4(tl.first, P.t[t], dp.t[t]), eps) * ec0.t[t];
        float c = dot<NT>(a0, Gc) * __builtin_amdgcn_rcpf(dot<NT>(a0, Rc));
        c = fmaxf(c, sum<NT>(Gv) * __builtin_amdgcn_rcpf(sum<NT>(Rv)));     // what the chunk before does not get
        // ... and what that share becomes under the last row of the chunk before (whose kernel starts from the chunk
        // scan's floor-free suffix vector)
        XT<NT> ep = zero_vec<NT>();
        if (tl.valid && tl.chain % p.C != 0) {               // (not the sequence's first chunk: the row exists)
            const char *pe = reinterpret_cast<const char *>(tl.baseE) + (tl.voff - rowb);
            XT<NT> raw;
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const f4u r = *reinterpret_cast<const f4u *>(pe + 64 * t);
                raw.t[t] = (f4){r.x, r.y, r.z, r.w};
            }
            ep = clamp<NT>(raw, bd);
        }
        const float dn = dot<NT>(ep, Rv);
        c = fmaxf(c, dn > 0.f ? dot<NT>(ep, Gv) * __builtin_amdgcn_rcpf(dn) : 0.f);
        if (g == 0 && tl.valid) phi[tl.chain] = c;
    }
}

// need[seq] = 1: the serial kernels (hmm_midq.inc) compute this sequence — its model is not served by the
// chunked scan, or its certificate (phi summed over its chunks: psi of the posterior, the one-directional CERT /
// CERT3 sums of hmm_forward / hmm_backward) is above EXACT_DELTA, or a reduce marked one of its chains: the
// operator columns went through the denormal range, or every column met an observation it survives at the emission
// floor only.  The sparse reduce keeps that mark in the pad lane of the exponent row (rows of W ints; 29 < W
// states), the dense reduces in risk[chain] (any q up to W).
__global__ __launch_bounds__(256) void k_scan_select(const int *__restrict__ elig, const float *__restrict__ phi,
                                                     int *__restrict__ need, int *__restrict__ nex, Plan p, float eps,
                                                     int exact_mode, const int *__restrict__ exps,
                                                     const int *__restrict__ risk, int W) {
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
        const bool dense = elig_dense(el);
        for (int c = 0; c < p.C; ++c) {
            const size_t chain = (size_t)seq * p.C + c;
            f = f || (dense ? risk[chain] != 0 : exps[chain * W + W - 1] != 0);
        }
    }
    need[seq] = f ? 1 : 0;
    if (f) atomicAdd(nex, 1);
}
