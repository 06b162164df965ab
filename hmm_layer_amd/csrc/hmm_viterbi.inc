// hmm_viterbi.inc — max-plus (Viterbi) scan, included at the end of hmm_engine.hip.
//
// The reference has no Viterbi (hmm_layer/MsaHmmCell.py:13 mentions it, :46-47 builds an unused
// log A); semantics are defined by oracle/viterbi.py: scores are Q16 fixed point,
//     Q(x) = rint(clip(x, -1024, 1024) * 65536),
// d_t[j] = max_i(d_{t-1}[i] + Q(logA[i,j])) + Q(logE_t[j]), lowest-index tie-breaks.  Integer
// max-plus is exactly associative, so the chunked scan below yields the same integers and the
// same path as the serial recursion BY CONSTRUCTION.  Every term is bounded by 2^26, and any state
// can be reached from the previous step's best state at a bounded cost, so the spread of scores
// within one step is < 2^29: 32-bit values relative to the per-step maximum plus a 64-bit base
// are exact — nothing saturates.
//
// Kernels (same chunking as the posterior pipeline, chunk operators in the max-plus semiring):
//   k_vit_prep      Q(logA), Q(logpi) and a CSR edge list per model: entries equal to the matrix
//                   minimum ("approximately log zero", absent edges) are not edges — they are all
//                   covered by ONE candidate (best previous state + minimum), which is exact.
//   k_vit_reduce    lane = (chain, start state): the chunk operator V[i][k], 4 chains per wave.
//   k_vit_scan_fwd  per sequence: scores entering every chunk, final state and score.
//   k_vit_apply     lane = (chain, state): true scores inside the chunk, 4-bit backpointers
//                   (8 bytes per position) and the map "state at chunk end -> state before chunk".
//   k_vit_scan_bwd  per sequence: state at every chunk end.
//   k_vit_backtrace lane = chain: follows the backpointers inside each chunk, writes the path.

#define VQ_CLAMP 1024.0f
#define VQ_SCALE 65536.0f
#define VT 16            // steps per LDS tile (== SP_TILE)
#define VR_NORM 8        // k_vit_reduce_sparse moves its score frame every VR_NORM steps (power of two, divides VT)

// backpointer word (8 B per position of a chain) of (chain, step t): chains interleaved in groups of 64
__device__ __forceinline__ size_t vit_bp_index(long long chain, int t, int T) {
    return ((size_t)(chain >> 6) * T + t) * 64 + (size_t)(chain & 63);
}

__device__ __forceinline__ int vquant(float v) {
    v = (v > -VQ_CLAMP) ? v : -VQ_CLAMP;          // also -inf and NaN -> -1024
    v = (v < VQ_CLAMP) ? v : VQ_CLAMP;
    return (int)__builtin_rintf(v * VQ_SCALE);
}

#ifndef HMM_VIT_NT
#define HMM_VIT_NT 0
#endif
struct VModel {               // per model, in the workspace
    int aq[QP * QP];          // Q(logA[i][j]) at [i*QP + j]
    int p0[QP];               // Q(logpi)
    int rowptr[QP + 1];       // CSR by destination j
    int src[QP * QP];
    int wgt[QP * QP];
    int a_off;                // matrix minimum: value of every entry that is not in the edge list
    int nnz;
    int topo;                 // ID of a compiled-in topology containing every edge, 0 = none
    int unit;                 // 1: every single-successor state of that topology carries Q(log 1) = 0 on its edge
};

struct VPlan {
    Plan p;
    size_t o_model, o_vops, o_vbase, o_dstart, o_dbase, o_forig, o_send, o_sfinal, o_bp, total;
    // two-level chunk scans (p.G groups of p.gsize chunks per sequence, as in the posterior pipeline)
    size_t o_gvops, o_gvbase, o_gdstart, o_gdbase, o_gforig, o_gsend;
};

static int make_vplan(int b, int L, int q, VPlan *v) {      // one model at a time
    // choose_T's chunk, not the posterior plans' round-aware one: that rule is fitted to k_forward / k_backward
    int rc = make_plan(HMM_OP_LOGLIK, 1, b, L, q, &v->p, choose_T(b, L));
    if (rc) return rc;
    const Plan &p = v->p;
    size_t off = 0;
    v->o_model = off;  off = align_up(off + sizeof(VModel));
    v->o_vops = off;   off = align_up(off + (size_t)p.nchains * QP * QP * sizeof(int));
    v->o_vbase = off;  off = align_up(off + (size_t)p.nchains * QP * sizeof(long long));
    v->o_dstart = off; off = align_up(off + (size_t)p.nchains * QP * sizeof(int));
    v->o_dbase = off;  off = align_up(off + (size_t)p.nchains * sizeof(long long));
    v->o_forig = off;  off = align_up(off + (size_t)p.nchains * QP);
    v->o_send = off;   off = align_up(off + (size_t)p.nchains * sizeof(int));
    v->o_sfinal = off; off = align_up(off + (size_t)p.NB * sizeof(int));
    const size_t ng = (size_t)p.NB * (p.G > 0 ? p.G : 1);
    v->o_gvops = off;   off = align_up(off + ng * QP * QP * sizeof(int));
    v->o_gvbase = off;  off = align_up(off + ng * QP * sizeof(long long));
    v->o_gdstart = off; off = align_up(off + ng * QP * sizeof(int));
    v->o_gdbase = off;  off = align_up(off + ng * sizeof(long long));
    v->o_gforig = off;  off = align_up(off + ng * QP);
    v->o_gsend = off;   off = align_up(off + ng * sizeof(int));
    // backpointer words (8 B per position of a chain), interleaved by groups of 64 chains:
    // word of (chain, step t) at ((chain / 64) * T + t) * 64 + chain % 64 — the lane-per-chain kernels
    // (k_vit_apply_sparse, k_vit_backtrace) write / read 512 contiguous bytes per step
    v->o_bp = off;     off = align_up(off + (size_t)((p.nchains + 63) / 64) * 64 * p.T * sizeof(unsigned long long));
    v->total = off;
    return HMM_OK;
}

template <class T>
__device__ bool edges_fit(const VModel &M, int q) {     // every explicit edge is an edge of T
    if (q != T::Q) return false;
    for (int j = 0; j < T::Q; ++j)
        for (int e = M.rowptr[j]; e < M.rowptr[j + 1]; ++e) {
            bool ok = false;
            for (int f = T::start[j]; f < T::start[j + 1]; ++f) ok = ok || (T::src[f] == M.src[e]);
            if (!ok) return false;
        }
    return true;
}

// every state of T with a single outgoing edge has weight Q(log 1) = 0 on it (a softmax over one edge)
template <class T>
__device__ int zero_single_edges(const VModel &M) {
    for (int j = 0; j < T::Q; ++j)
        for (int e = T::start[j]; e < T::start[j + 1]; ++e)
            if (out_degree<T>(T::src[e]) == 1 && M.aq[T::src[e] * QP + j] != 0) return 0;
    return 1;
}

__global__ void k_vit_prep(const float *__restrict__ logA, const float *__restrict__ logpi, VModel *models, int q,
                           int force_generic) {
    const int m = 0;
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    VModel &M = models[m];
    int amin = 0x7fffffff;
    for (int i = 0; i < QP; ++i)
        for (int j = 0; j < QP; ++j) {
            int v = (i < q && j < q) ? vquant(logA[((size_t)m * q + i) * q + j]) : 0;
            M.aq[i * QP + j] = v;
            if (i < q && j < q && v < amin) amin = v;
        }
    for (int j = 0; j < QP; ++j) M.p0[j] = (j < q) ? vquant(logpi[(size_t)m * q + j]) : 0;
    int n = 0;
    for (int j = 0; j < QP; ++j) {
        M.rowptr[j] = n;
        if (j < q)
            for (int i = 0; i < q; ++i)
                if (M.aq[i * QP + j] > amin) { M.src[n] = i; M.wgt[n] = M.aq[i * QP + j]; ++n; }
    }
    M.rowptr[QP] = n;
    M.a_off = amin;
    M.nnz = n;
    M.topo = force_generic ? 0 : (edges_fit<TopoGene15>(M, q) ? TopoGene15::ID : (edges_fit<TopoGene7>(M, q) ? TopoGene7::ID : 0));
    M.unit = M.topo == TopoGene15::ID ? zero_single_edges<TopoGene15>(M) : (M.topo == TopoGene7::ID ? zero_single_edges<TopoGene7>(M) : 0);
}

// ---- shared emission staging for the two lane-per-(chain, x) kernels: 4 chains per wave, tiles of
// VT steps, quantised once while staging.  LDS image per chain: [step][16 ints], padded stride.
struct VStage {
    __amdgpu_buffer_rsrc_t rs;
    int coff[4];
    int loff[4];
    bool loader;
    int q;
};

__device__ __forceinline__ VStage make_vstage(const float *logE, const Plan &p, long long wchain0, int lane) {
    VStage s;
    const int q = p.q;
    s.q = q;
    const long long seq0 = wchain0 / p.C;
    const long long row0 = seq0 * p.L + (wchain0 - seq0 * p.C) * (long long)p.T;
    const unsigned long long total = (unsigned long long)p.NB * p.L * q * sizeof(float);
    s.rs = make_rsrc(logE + row0 * q, total - (unsigned long long)row0 * q * sizeof(float));
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        long long ch = wchain0 + j;
        if (ch >= p.nchains) ch = wchain0;
        const long long sq = ch / p.C;
        const long long rw = sq * p.L + (ch - sq * p.C) * (long long)p.T;
        s.coff[j] = (int)((rw - row0) * q * (long long)sizeof(float));
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int idx = 4 * lane + u;
        s.loff[u] = (idx / q) * QP + (idx % q);
    }
    s.loader = lane < (VT * q + 3) / 4;
    return s;
}
#define VCH (VT * QP + 16)        // ints per chain image (padded)

__device__ __forceinline__ void vfetch(const VStage &s, int tile, int lane, f4 (&r)[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
        r[j] = __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(
            s.rs, s.coff[j] + tile * (VT * s.q * 4) + lane * 16, 0, 0));
}
__device__ __forceinline__ void vstage(const VStage &s, int lane, const f4 (&r)[4], int *tile_lds /*[4][VCH]*/) {
    if (!s.loader) return;
    const int nfl = VT * s.q - 4 * lane;                 // floats of this piece inside the tile
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        int *dst = tile_lds + j * VCH;
        if (nfl > 0) dst[s.loff[0]] = vquant(r[j].x);
        if (nfl > 1) dst[s.loff[1]] = vquant(r[j].y);
        if (nfl > 2) dst[s.loff[2]] = vquant(r[j].z);
        if (nfl > 3) dst[s.loff[3]] = vquant(r[j].w);
    }
}

// ------------------------------------------------------------------ reduce (max-plus operators)
__global__ __launch_bounds__(256) void k_vit_reduce(const float *__restrict__ logE, const VModel *__restrict__ models,
                                                    int *__restrict__ vops, long long *__restrict__ vbase, Plan p) {
    __shared__ int etile[4][2][4][VCH];
    __shared__ int xs[4][2][QP][64];                     // [wave][buffer][state][lane]
    __shared__ int esrc[QP * QP], ewgt[QP * QP], erow[QP + 1];
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63, cl = lane >> 4, kc = lane & 15;
    const long long wchain0 = ((long long)blockIdx.x * 4 + w) * 4;
    const int q = p.q;
    const VModel &M = models[0];                         // the host launches one model at a time
    for (int i = threadIdx.x; i < QP * QP; i += 256) { esrc[i] = M.src[i]; ewgt[i] = M.wgt[i]; }
    if (threadIdx.x <= QP) erow[threadIdx.x] = M.rowptr[threadIdx.x];
    const int a_off = M.a_off;
    if (M.topo != 0) return;                              // k_vit_reduce_sparse serves this model
    __syncthreads();
    if (wchain0 >= p.nchains) return;
    const long long chain = wchain0 + cl;
    const bool inrange = chain < p.nchains;
    const long long chn = inrange ? chain : wchain0;
    const int seq = (int)(chn / p.C), c = (int)(chn - (long long)seq * p.C);
    const int len = inrange ? min(p.T, p.L - c * p.T) : 0;
    const bool first = (c == 0) && p.seq_start;        // (a later time slab's chunk 0 is an ordinary chunk)
    const VStage st = make_vstage(logE, p, wchain0, lane);
    int *xw = &xs[w][0][0][0];
    // column kc of the identity in the max-plus sense is not representable with bounded spread;
    // the recursion therefore starts AFTER the first step: x = A[kc][.] + E_t0 for an ordinary
    // chunk, pi + E_0 (the same in every column) for the first chunk of a sequence
    f4 r[4];
    vfetch(st, 0, lane, r);
    int cur = 0;
    long long base = 0;
    int mprev = 0;
    const int ntiles = p.T / VT;
    const int last = len - 1;
    for (int tile = 0; tile < ntiles; ++tile) {
        const int buf = tile & 1;
        vstage(st, lane, r, &etile[w][buf][0][0]);
        if (tile + 1 < ntiles) vfetch(st, tile + 1, lane, r);
        const int *et = &etile[w][buf][cl][0];
        for (int sidx = 0; sidx < VT; ++sidx) {
            const int t = tile * VT + sidx;
            int mx = -0x7fffffff;
            int *xc = xw + cur * QP * 64, *xn = xw + (cur ^ 1) * QP * 64;
            if (t == 0) {
                for (int j = 0; j < q; ++j) {
                    const int y = (first ? M.p0[j] : M.aq[(kc < q ? kc : 0) * QP + j]) + et[j];
                    xn[j * 64 + lane] = y;
                    mx = max(mx, y);
                }
            } else {
                for (int j = 0; j < q; ++j) {
                    int best = -0x40000000;           // below every real candidate, no overflow in best - mprev
                    for (int e = erow[j]; e < erow[j + 1]; ++e) best = max(best, xc[esrc[e] * 64 + lane] + ewgt[e]);
                    // stored values are relative to the previous-previous maximum: the previous
                    // maximum (mprev) becomes 0, so "best previous state + a_off" is just a_off
                    const int y = max(best - mprev, a_off) + et[sidx * QP + j];
                    xn[j * 64 + lane] = y;
                    mx = max(mx, y);
                }
            }
            base += mx;
            mprev = mx;
            cur ^= 1;
            if (__builtin_amdgcn_ballot_w64(t == last) != 0) {
                if (t == last && kc < q) {
                    const int *xf = xw + cur * QP * 64;
                    for (int j = 0; j < QP; ++j) vops[(size_t)chain * QP * QP + j * QP + kc] = (j < q) ? xf[j * 64 + lane] - mx : 0;
                    vbase[(size_t)chain * QP + kc] = base;
                }
            }
        }
    }
}

// ------------------------------------------------------------------ reduce, compiled-in topologies
// Same operators as k_vit_reduce with the column in registers and the structural edges unrolled
// (the generic kernel keeps the column in LDS and walks a runtime edge list: 41 ms vs ~3 ms on
// b=1024 x L=1e5).  Every edge of T is evaluated with its actual weight — edges of T that are
// "absent" in this model simply carry the matrix minimum, which the catch-all candidate dominates.
// UNIT: the single-successor states' edges weigh 0 (VModel::unit): their candidate is the source's score itself
typedef int VrLds[4][2][4][VCH];
template <class T, bool UNIT>
__device__ __forceinline__ void vit_reduce_sparse_body(const float *__restrict__ logE, const VModel &M,
                                                       int *__restrict__ vops, long long *__restrict__ vbase,
                                                       const Plan &p, VrLds &etile) {
    constexpr int Q = T::Q;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63, cl = lane >> 4, kc = lane & 15;
    const long long wchain0 = ((long long)blockIdx.x * 4 + w) * 4;
    if (wchain0 >= p.nchains) return;
    auto cand = [&](const int (&xv)[Q], const int (&av)[T::NE], int ed) {
        const int i = T::src[ed];
        return (UNIT && out_degree<T>(i) == 1) ? xv[i] : xv[i] + av[ed];
    };
    const long long chain = wchain0 + cl;
    const bool inrange = chain < p.nchains;
    const long long chn = inrange ? chain : wchain0;
    const int seq = (int)(chn / p.C), c = (int)(chn - (long long)seq * p.C);
    const int len = inrange ? min(p.T, p.L - c * p.T) : 0;
    const bool first = (c == 0) && p.seq_start;        // (a later time slab's chunk 0 is an ordinary chunk)
    const int a_off = M.a_off;
    int a[T::NE];
#pragma unroll
    for (int j = 0; j < Q; ++j)
#pragma unroll
        for (int e = T::start[j]; e < T::start[j + 1]; ++e) a[e] = M.aq[T::src[e] * QP + j];
    const VStage st = make_vstage(logE, p, wchain0, lane);
    for (int i = lane; i < 2 * 4 * VCH; i += 64) (&etile[w][0][0][0])[i] = 0;
    f4 r[4];
    vfetch(st, 0, lane, r);
    int x[Q];
    long long base = 0;          // true score = x[j] + base; the frame moves only every VR_NORM steps:
    int mprev = 0;               // per-step values stay within 2^29 (spread) + VR_NORM * 2^27 < 2^31
    const int last = len - 1;
    const int ntiles = p.T / VT;
    auto finish = [&](int mx) {
        if (kc < Q) {
#pragma unroll
            for (int j = 0; j < Q; ++j) vops[(size_t)chain * QP * QP + j * QP + kc] = x[j] - mx;
#pragma unroll
            for (int j = Q; j < QP; ++j) vops[(size_t)chain * QP * QP + j * QP + kc] = 0;
            vbase[(size_t)chain * QP + kc] = base + mx;
        }
    };
    for (int tile = 0; tile < ntiles; ++tile) {
        const int buf = tile & 1;
        vstage(st, lane, r, &etile[w][buf][0][0]);
        if (tile + 1 < ntiles) vfetch(st, tile + 1, lane, r);
        const int *et = &etile[w][buf][cl][0];
#pragma unroll 8
        for (int sidx = 0; sidx < VT; ++sidx) {
            const i4 *er = reinterpret_cast<const i4 *>(et + sidx * QP);
            const i4 e0 = er[0], e1 = er[1], e2 = er[2], e3 = er[3];
            const int e[16] = {e0.x, e0.y, e0.z, e0.w, e1.x, e1.y, e1.z, e1.w, e2.x, e2.y, e2.z, e2.w, e3.x, e3.y, e3.z, e3.w};
            int y[Q];
            int mx = -0x7fffffff;
            if (tile == 0 && sidx == 0) {                 // wave-uniform: first step of every chunk
#pragma unroll
                for (int j = 0; j < Q; ++j) {
                    y[j] = (first ? M.p0[j] : M.aq[(kc < Q ? kc : 0) * QP + j]) + e[j];
                    mx = max(mx, y[j]);
                }
            } else {
                // every source that is not an explicit edge: the best previous score at the matrix minimum
                const int rest = mprev + a_off;
#pragma unroll
                for (int j = 0; j < Q; ++j) {
                    int best = cand(x, a, T::start[j]);
#pragma unroll
                    for (int ed = T::start[j] + 1; ed < T::start[j + 1]; ++ed) best = max(best, cand(x, a, ed));
                    y[j] = max(best, rest) + e[j];
                    mx = max(mx, y[j]);
                }
            }
            const int t = tile * VT + sidx;
            if ((sidx & (VR_NORM - 1)) == VR_NORM - 1) {   // compile-time after unrolling: move the frame
#pragma unroll
                for (int j = 0; j < Q; ++j) x[j] = y[j] - mx;
                base += mx;
                mprev = 0;
                if (__builtin_amdgcn_ballot_w64(t == last) != 0) { if (t == last) finish(0); }
            } else {
#pragma unroll
                for (int j = 0; j < Q; ++j) x[j] = y[j];
                mprev = mx;
                if (__builtin_amdgcn_ballot_w64(t == last) != 0) { if (t == last) finish(mx); }
            }
        }
    }
}

template <class T>
// held to 3 waves per SIMD (LDS alone would allow 4): no slower by itself, and it leaves registers and LDS for
// one wave per SIMD of the in-chunk pass of the previous batch group (see vit_groups)
#ifndef HMM_VRS_WPE
#define HMM_VRS_WPE 3
#endif
#define VRS_ATTR __attribute__((amdgpu_waves_per_eu(HMM_VRS_WPE, HMM_VRS_WPE)))
__global__ __launch_bounds__(256) VRS_ATTR void k_vit_reduce_sparse(const float *__restrict__ logE, const VModel *__restrict__ models,
                                                           int *__restrict__ vops, long long *__restrict__ vbase, Plan p) {
    __shared__ __attribute__((aligned(16))) VrLds etile;
    const VModel &M = models[0];
    if (M.topo != T::ID) return;
    if (M.unit) vit_reduce_sparse_body<T, true>(logE, M, vops, vbase, p, etile);
    else vit_reduce_sparse_body<T, false>(logE, M, vops, vbase, p, etile);
}

// ------------------------------------------------------------------ forward scan over chunk operators
// 16 lanes, lane i = state.  Walks the operators of chunks [c_from, c_to) of one sequence: before
// every chunk c in (c_from, c_to) it records the scores entering it (relative to their maximum, + base);
// d = true scores entering chunk c_from + 1, i.e. after chunk c_from.  Returns the scores after chunk
// c_to - 1.  The next hop's operator row and bases are fetched one hop ahead (a dependent 200-byte load
// per hop and sixteen LDS-routed shuffles made a hop 2.7 us); broadcasts are v_readlane.
__device__ __forceinline__ long long vit_hops(const int *__restrict__ vops, const long long *__restrict__ vbase,
                                              int *__restrict__ dstart, long long *__restrict__ dbase, size_t chain0,
                                              int c_from, int c_to, long long d, int i, int q) {
    i4 v0 = {0, 0, 0, 0}, v1 = v0, v2 = v0, v3 = v0;
    long long vbn = 0;
    auto fetch = [&](int c) {
        const i4 *V = reinterpret_cast<const i4 *>(vops + (chain0 + c) * QP * QP + i * QP);
        v0 = V[0]; v1 = V[1]; v2 = V[2]; v3 = V[3];
        vbn = vbase[(chain0 + c) * QP + i];                 // base of column i: lane i holds it, broadcast per term
    };
    if (c_from + 1 < c_to) fetch(c_from + 1);
    for (int c = c_from + 1; c < c_to; ++c) {
        // normalise: relative scores (max = 0) + base
        long long mx = (i < q) ? d : (long long)0x8000000000000000ll;
        for (int s = 1; s < 16; s <<= 1) { long long o = __shfl_xor(mx, s, 16); mx = o > mx ? o : mx; }
        const int rel = (i < q) ? (int)(d - mx) : 0;
        dstart[(chain0 + c) * QP + i] = rel;
        if (i == 0) dbase[chain0 + c] = mx;
        // hop: d'[i] = max_k (rel[k] + V[i][k] + vbase[k]) + mx
        const int vr[16] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w, v2.x, v2.y, v2.z, v2.w, v3.x, v3.y, v3.z, v3.w};
        const long long vb = vbn;
        if (c + 1 < c_to) fetch(c + 1);
        const int vblo = (int)(unsigned)(vb & 0xffffffffll), vbhi = (int)(vb >> 32);
        long long best = (long long)0x8000000000000000ll;
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) {
            const long long bk = ((long long)__builtin_amdgcn_readlane(vbhi, kk) << 32) |
                                 (long long)(unsigned)__builtin_amdgcn_readlane(vblo, kk);
            const long long cand = (long long)__builtin_amdgcn_readlane(rel, kk) + (long long)vr[kk] + bk;
            best = (kk < q && cand > best) ? cand : best;
        }
        d = best + mx;
    }
    return d;
}

// final state (lowest index with the maximal score) and score of a sequence from its last scores
__device__ __forceinline__ void vit_final(long long d, int i, int q, int seq, int *__restrict__ sfinal,
                                          double *__restrict__ score) {
    long long mx = (i < q) ? d : (long long)0x8000000000000000ll;
    for (int s = 1; s < 16; s <<= 1) { long long o = __shfl_xor(mx, s, 16); mx = o > mx ? o : mx; }
    unsigned long long ball = __builtin_amdgcn_ballot_w64(i < q && d == mx);
    if (i == 0) { sfinal[seq] = __builtin_ctzll(ball); score[seq] = (double)mx / (double)VQ_SCALE; }
}

// one sequence per block: all C operators in order (single level), or the G group operators of the
// two-level scan (then dstart / dbase are the groups' and C = G)
__global__ __launch_bounds__(64) void k_vit_scan_fwd(const int *__restrict__ vops, const long long *__restrict__ vbase,
                                                     int *__restrict__ dstart, long long *__restrict__ dbase,
                                                     int *__restrict__ sfinal, double *__restrict__ score, Plan p) {
    const int seq = blockIdx.x;
    const int i = threadIdx.x;
    if (i >= 16) return;
    const int q = p.q, C = p.C;
    const size_t chain0 = (size_t)seq * C;
    // chunk 0: every column holds the true score vector
    long long d = (i < q) ? (long long)vops[chain0 * QP * QP + i * QP + 0] + vbase[chain0 * QP + 0] : 0;
    d = vit_hops(vops, vbase, dstart, dbase, chain0, 0, C, d, i, q);
    vit_final(d, i, q, seq, sfinal, score);
}

// ---- two-level forward scan.  Integer max-plus composes exactly, so groups of ~sqrt(C) chunk operators
// are composed in parallel (k_vit_scan_compose), k_vit_scan_fwd walks the G group operators, and
// k_vit_scan_inner walks the chunks of every group in parallel from the group's entry scores: ~3 sqrt(C)
// dependent hops instead of C (one sequence of 1e6 positions: 1954 -> 135).
//
// One wave per (sequence, group): W <- V_c (x) W over the group's chunks, W = V_{c0} at the start.
// Lane (k = lane & 15, ig = lane >> 4) owns rows 4 ig .. 4 ig + 3 of column k; the current W goes
// through LDS so that every lane can read its whole column.  All sums in 64 bits; every column leaves
// normalised (maximum 0) with its own base, the format of the chunk operators.
__global__ __launch_bounds__(256) void k_vit_scan_compose(const int *__restrict__ vops, const long long *__restrict__ vbase,
                                                          int *__restrict__ gvops, long long *__restrict__ gvbase, Plan p) {
    __shared__ int wl[4][QP][QP + 1];               // [wave][m][k] relative scores
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long wv = (long long)blockIdx.x * 4 + w;
    if (wv >= (long long)p.NB * p.G) return;
    const int lane = threadIdx.x & 63, k = lane & 15, ig = lane >> 4;
    const int seq = (int)(wv / p.G), grp = (int)(wv - (long long)seq * p.G);
    const int c0 = grp * p.gsize, c1 = min(p.C, c0 + p.gsize);
    const int q = p.q;
    const size_t ch0 = (size_t)seq * p.C + c0;
    int wr[4];                                      // W[4 ig + r][k], relative to the column's base
#pragma unroll
    for (int r = 0; r < 4; ++r) wr[r] = vops[ch0 * QP * QP + (4 * ig + r) * QP + k];
    long long wb = vbase[ch0 * QP + k];
    for (int c = c0 + 1; c < c1; ++c) {
        const size_t ch = (size_t)seq * p.C + c;
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int r = 0; r < 4; ++r) wl[w][4 * ig + r][k] = wr[r];
        __builtin_amdgcn_wave_barrier();
        long long best[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) best[r] = (long long)0x8000000000000000ll;
        int vrow[4][QP];                            // rows 4 ig .. 4 ig + 3 of V_c
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const i4 t4 = *reinterpret_cast<const i4 *>(vops + ch * QP * QP + (4 * ig + r) * QP + 4 * u);
                vrow[r][4 * u] = t4.x; vrow[r][4 * u + 1] = t4.y; vrow[r][4 * u + 2] = t4.z; vrow[r][4 * u + 3] = t4.w;
            }
#pragma unroll
        for (int m = 0; m < QP; ++m) {
            if (m >= q) continue;                   // wave-uniform
            const long long t = (long long)wl[w][m][k] + vbase[ch * QP + m];      // W[m][k] (rel) + base of V_c's column m
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long long cand = t + (long long)vrow[r][m];
                best[r] = cand > best[r] ? cand : best[r];
            }
        }
        // column maximum over the 16 rows: 4 in this lane, 4 lanes per column (16 apart)
        long long mx = (long long)0x8000000000000000ll;
#pragma unroll
        for (int r = 0; r < 4; ++r) mx = (4 * ig + r < q && best[r] > mx) ? best[r] : mx;
        { long long o = __shfl_xor(mx, 16); mx = o > mx ? o : mx; }
        { long long o = __shfl_xor(mx, 32); mx = o > mx ? o : mx; }
#pragma unroll
        for (int r = 0; r < 4; ++r) wr[r] = (4 * ig + r < q && k < q) ? (int)(best[r] - mx) : 0;
        wb = k < q ? wb + mx : 0;
    }
#pragma unroll
    // (a group of one chunk is that chunk's operator, whose columns from q on were never written: they leave as 0)
    for (int r = 0; r < 4; ++r) gvops[(size_t)wv * QP * QP + (4 * ig + r) * QP + k] = k < q ? wr[r] : 0;
    if (ig == 0) gvbase[(size_t)wv * QP + k] = k < q ? wb : 0;
}

// one block per (sequence, group): the hops of the single-level scan over the group's chunks, from the
// scores entering the group (gdstart / gdbase; group 0 starts at the sequence's first chunk itself)
__global__ __launch_bounds__(64) void k_vit_scan_inner(const int *__restrict__ vops, const long long *__restrict__ vbase,
                                                       const int *__restrict__ gdstart, const long long *__restrict__ gdbase,
                                                       int *__restrict__ dstart, long long *__restrict__ dbase, Plan p) {
    const long long blk = blockIdx.x;
    const int i = threadIdx.x;
    if (i >= 16) return;
    const int q = p.q;
    const int seq = (int)(blk / p.G), grp = (int)(blk - (long long)seq * p.G);
    const int c0 = grp * p.gsize, c1 = min(p.C, c0 + p.gsize);
    const size_t chain0 = (size_t)seq * p.C;
    long long d;
    if (grp == 0 && p.seq_start) {
        d = (i < q) ? (long long)vops[chain0 * QP * QP + i * QP + 0] + vbase[chain0 * QP + 0] : 0;
    } else {
        // scores entering chunk c0: recorded for the chunk itself, then through its operator
        const int rel = gdstart[(size_t)blk * QP + i];
        const long long mx = gdbase[blk];
        dstart[(chain0 + c0) * QP + i] = rel;
        if (i == 0) dbase[chain0 + c0] = mx;
        long long best = (long long)0x8000000000000000ll;
        for (int kk = 0; kk < q; ++kk) {
            const long long cand = (long long)__builtin_amdgcn_readlane(rel, kk) +
                                   (long long)vops[(chain0 + c0) * QP * QP + i * QP + kk] + vbase[(chain0 + c0) * QP + kk];
            best = cand > best ? cand : best;
        }
        d = best + mx;
    }
    (void)vit_hops(vops, vbase, dstart, dbase, chain0, c0, c1, d, i, q);
}

// ------------------------------------------------------------------ apply: true scores, backpointers
__global__ __launch_bounds__(256) void k_vit_apply(const float *__restrict__ logE, const VModel *__restrict__ models,
                                                   const int *__restrict__ dstart, unsigned char *__restrict__ forig,
                                                   unsigned int *__restrict__ bp, Plan p) {
    __shared__ int etile[4][2][4][VCH];
    __shared__ int xs[4][4][QP];                         // [wave][chain][state] scores relative to the max
    __shared__ int og[4][2][4][QP];                      // [wave][buffer][chain][state] origin before the chunk
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63, cl = lane >> 4, j = lane & 15;
    const long long wchain0 = ((long long)blockIdx.x * 4 + w) * 4;
    const int q = p.q;
    const VModel &M = models[0];
    if (M.topo != 0) return;                              // k_vit_apply_sparse serves this model (uniform)
    __shared__ int esrc[QP * QP], ewgt[QP * QP];
    for (int i = threadIdx.x; i < QP * QP; i += 256) { esrc[i] = M.src[i]; ewgt[i] = M.wgt[i]; }
    __syncthreads();
    if (wchain0 >= p.nchains) return;
    const long long chain = wchain0 + cl;
    const bool inrange = chain < p.nchains;
    const long long chn = inrange ? chain : wchain0;
    const int seq = (int)(chn / p.C), c = (int)(chn - (long long)seq * p.C);
    const int t0 = c * p.T;
    const int len = inrange ? min(p.T, p.L - t0) : 0;
    const bool first = (c == 0) && p.seq_start;        // (a later time slab's chunk 0 is an ordinary chunk)
    const bool act_state = j < q;
    const int e0 = M.rowptr[j], e1 = M.rowptr[j + 1], a_off = M.a_off;
    const VStage st = make_vstage(logE, p, wchain0, lane);
    xs[w][cl][j] = (act_state && !first) ? dstart[(size_t)chn * QP + j] : (act_state ? 0 : -0x40000000);
    og[w][0][cl][j] = j;
    f4 r[4];
    vfetch(st, 0, lane, r);
    int ocur = 0;
    const int ntiles = p.T / VT;
    unsigned int *bpw = bp + vit_bp_index(chn, 0, p.T) * 2;          // step t: + t * 128 words
    for (int tile = 0; tile < ntiles; ++tile) {
        const int buf = tile & 1;
        vstage(st, lane, r, &etile[w][buf][0][0]);
        if (tile + 1 < ntiles) vfetch(st, tile + 1, lane, r);
        const int *et = &etile[w][buf][cl][0];
        for (int sidx = 0; sidx < VT; ++sidx) {
            const int t = tile * VT + sidx;
            const bool live = t < len;
            const int *xc = &xs[w][cl][0];
            int y, arg;
            if (first && t == 0) {
                y = M.p0[j] + et[j];
                arg = j;
            } else {
                // candidate standing for every source that is not an explicit edge: the lowest-index
                // best previous state (relative score 0) at the matrix minimum
                const unsigned long long ball = __builtin_amdgcn_ballot_w64(act_state && xc[j] == 0);
                const int istar = __builtin_ctz((unsigned)((ball >> (16 * cl)) & 0xffffu) | 0x10000u);
                long long best = ((long long)a_off << 4) | (long long)(15 - istar);
                for (int e = e0; e < e1; ++e) {
                    const int s = esrc[e];
                    const long long cand = ((long long)(xc[s] + ewgt[e]) << 4) | (long long)(15 - s);
                    best = cand > best ? cand : best;
                }
                y = (int)(best >> 4) + et[sidx * QP + j];
                arg = 15 - (int)(best & 15);
            }
            if (!act_state) y = -0x40000000;
            // renormalise the 16-lane row to max 0
            const int mx = row_max_i(y);
            // origin before the chunk of the best path into state j
            const int onew = (t == 0) ? arg : og[w][ocur][cl][arg];
            if (live) {
                xs[w][cl][j] = y - mx;
                og[w][ocur ^ 1][cl][j] = onew;
            }
            // 4-bit backpointers: states 0-7 -> word 0, 8-15 -> word 1
            unsigned v = act_state ? ((unsigned)arg << (4 * (j & 7))) : 0u;
            v |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, true);
            v |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, true);
            v |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xF, 0xF, true);
            if (live && (j & 7) == 0) bpw[(size_t)t * 128 + (j >> 3)] = v;
            if (live) ocur ^= 1;
        }
    }
    if (inrange && act_state) forig[(size_t)chain * QP + j] = (unsigned char)og[w][ocur][cl][j];
}

// ---- apply for the compiled-in topologies: lane = chain.  The in-chunk pass is a VECTOR recursion
// (Q scores per chain), so a lane can keep a whole chain in registers: scores, the packed origin map
// (4 bits per state) and the explicit edges as compile-time code — no LDS, no cross-lane traffic,
// 64 chains per wave.  Same integers, arguments and tie-breaks as k_vit_apply: explicit sources are
// visited in increasing index order with strict '>' (lowest index wins a tie), then the single
// "rest" candidate (lowest-index best previous state at the matrix minimum) is compared by
// (value, index).  (k_vit_apply, lane = (chain, state) through LDS: 4.2 ms at b=1024 x L=1e5.)
template <class T>
__host__ __device__ constexpr int vsorted_src(int j, int k) {      // k-th smallest source of destination j
    int prev = -1, cur = 0;
    for (int r = 0; r <= k; ++r) {
        cur = 1 << 20;
        for (int e = T::start[j]; e < T::start[j + 1]; ++e)
            if (T::src[e] > prev && T::src[e] < cur) cur = T::src[e];
        prev = cur;
    }
    return cur;
}

#define VA_TS 4           // steps per staged tile: 4 steps x q floats of a chain = exactly q 16-byte pieces
#define VA_LD (VA_TS * QP + 4)    // ints per chain in LDS (16-byte multiple; 4 lanes apart = 16 banks apart)

// Emissions reach the lanes through wave-private LDS: per tile the wave loads its 64 chains'
// 4-step spans (64 q contiguous 16-byte pieces, lane -> piece, a few cache lines per instruction),
// quantises them once and each lane reads back its own chain.  Letting every lane load its own rows
// instead (64 different cache lines per instruction, 5 instructions per step) saturated the L1:
// 3.8 ms whatever the occupancy.
template <class T>
__global__ __launch_bounds__(64) void k_vit_apply_sparse(const float *__restrict__ logE, const VModel *__restrict__ models,
                                                         const int *__restrict__ dstart,
                                                         unsigned char *__restrict__ forig,
                                                         unsigned long long *__restrict__ bp, Plan p) {
    constexpr int Q = T::Q;
    __shared__ __attribute__((aligned(16))) int tile[64 * VA_LD];
    __shared__ int chainoff[64];
    const VModel &M = models[0];
    if (M.topo != T::ID) return;
    const int lane = threadIdx.x;
    const long long wchain0 = (long long)blockIdx.x * 64;
    if (wchain0 >= p.nchains) return;
    const long long chain = wchain0 + lane;
    const bool inrange = chain < p.nchains;
    const long long chn = inrange ? chain : p.nchains - 1;
    const long long seq = chn / p.C;
    const int c = (int)(chn - seq * p.C);
    const int t0 = c * p.T;
    const int len = inrange ? min(p.T, p.L - t0) : 0;
    const bool first = (c == 0) && p.seq_start;        // (a later time slab's chunk 0 is an ordinary chunk)
    // emission rows: 32-bit offsets from the wave's first row, range-checked by the descriptor
    const long long seq0 = wchain0 / p.C;
    const long long row0 = seq0 * p.L + (wchain0 - seq0 * p.C) * p.T;
    const long long row = seq * p.L + t0;
    const unsigned long long total = (unsigned long long)p.NB * p.L * Q * sizeof(float);
    const __amdgpu_buffer_rsrc_t rs = make_rsrc(logE + row0 * Q, total - (unsigned long long)row0 * Q * sizeof(float));
    constexpr int rowb = Q * (int)sizeof(float);
    chainoff[lane] = (int)((row - row0) * rowb);
    // piece it*64 + lane of a tile belongs to chain pc[it], 16-byte piece pk[it] of its 4-step span
    int poff[Q], lds_w[Q];
#pragma unroll
    for (int it = 0; it < Q; ++it) {
        const int pidx = it * 64 + lane;
        const int pc = pidx / Q, pk = pidx - pc * Q;
        poff[it] = chainoff[pc] + 16 * pk;                 // own-wave LDS: written above, program order
        lds_w[it] = pc * VA_LD + 4 * pk;
    }
    // weights of the explicit edges (sources in increasing order), wave-uniform
    int a[T::NE > 0 ? T::NE : 1];
#pragma unroll
    for (int j = 0; j < Q; ++j)
#pragma unroll
        for (int k = 0; k < T::start[j + 1] - T::start[j]; ++k) a[T::start[j] + k] = M.aq[vsorted_src<T>(j, k) * QP + j];
    const int a_off = M.a_off;

    int x[Q];
#pragma unroll
    for (int j = 0; j < Q; ++j) x[j] = first ? 0 : dstart[(size_t)chn * QP + j];
    unsigned og_lo = 0x76543210u, og_hi = 0xfedcba98u;    // origin before the chunk of the best path into state j
    unsigned long long *bpc = bp + vit_bp_index(chn, 0, p.T);        // step t: + t * 64
    const int *mine = tile + lane * VA_LD;

    f4 pr[Q];
#pragma unroll
    for (int it = 0; it < Q; ++it)
        pr[it] = __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(rs, poff[it], 0, 0));
    const int ntile = p.T / VA_TS;
    for (int tl = 0; tl < ntile; ++tl) {
        __builtin_amdgcn_wave_barrier();                    // the previous tile's reads precede these writes
#pragma unroll
        for (int it = 0; it < Q; ++it) {
            const i4 v = {vquant(pr[it].x), vquant(pr[it].y), vquant(pr[it].z), vquant(pr[it].w)};
            *reinterpret_cast<i4 *>(tile + lds_w[it]) = v;
        }
        if (tl + 1 < ntile) {
#pragma unroll
            for (int it = 0; it < Q; ++it)
                pr[it] = __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(rs, poff[it] + (tl + 1) * VA_TS * rowb, 0, 0));
        }
        __builtin_amdgcn_wave_barrier();
        unsigned long long bpv[VA_TS];
#pragma unroll
        for (int u = 0; u < VA_TS; ++u) {
            const int t = tl * VA_TS + u;
            int e[Q];
#pragma unroll
            for (int j = 0; j < Q; ++j) e[j] = mine[u * Q + j];
            // lowest-index best previous state (scores are relative: the best is 0)
            int istar = Q - 1;
#pragma unroll
            for (int j = Q - 2; j >= 0; --j) istar = (x[j] == 0) ? j : istar;
            int y[Q], arg[Q];
#pragma unroll
            for (int j = 0; j < Q; ++j) {
                int best = x[vsorted_src<T>(j, 0)] + a[T::start[j]];
                int ar = vsorted_src<T>(j, 0);
#pragma unroll
                for (int k = 1; k < T::start[j + 1] - T::start[j]; ++k) {
                    const int cand = x[vsorted_src<T>(j, k)] + a[T::start[j] + k];
                    ar = cand > best ? vsorted_src<T>(j, k) : ar;
                    best = cand > best ? cand : best;
                }
                const bool take = a_off > best || (a_off == best && istar < ar);
                best = take ? a_off : best;
                ar = take ? istar : ar;
                y[j] = best + e[j];
                arg[j] = ar;
            }
            if (t == 0) {                                   // wave-uniform
#pragma unroll
                for (int j = 0; j < Q; ++j) {
                    y[j] = first ? M.p0[j] + e[j] : y[j];
                    arg[j] = first ? j : arg[j];
                }
            }
            int mx = y[0];
#pragma unroll
            for (int j = 1; j < Q; ++j) mx = max(mx, y[j]);
            unsigned nlo = 0, nhi = 0, blo = 0, bhi = 0;
#pragma unroll
            for (int j = 0; j < Q; ++j) {
                const unsigned ar = (unsigned)arg[j];
                const unsigned o = (((ar & 8u) ? og_hi : og_lo) >> (4 * (ar & 7u))) & 15u;
                if (j < 8) { nlo |= o << (4 * j); blo |= ar << (4 * j); }
                else { nhi |= o << (4 * (j - 8)); bhi |= ar << (4 * (j - 8)); }
            }
            bpv[u] = (unsigned long long)blo | ((unsigned long long)bhi << 32);
            if (t < len) {
#pragma unroll
                for (int j = 0; j < Q; ++j) x[j] = y[j] - mx;
                og_lo = nlo; og_hi = nhi;
            }
        }
        // this tile's backpointers: per step the wave's 64 words are 512 contiguous bytes
        const int tb = tl * VA_TS;
#pragma unroll
        for (int u = 0; u < VA_TS; ++u)
#if HMM_VIT_NT
            if (tb + u < len) __builtin_nontemporal_store(bpv[u], &bpc[(size_t)(tb + u) * 64]);
#else
            if (tb + u < len) bpc[(size_t)(tb + u) * 64] = bpv[u];
#endif
    }
    if (inrange) {
#pragma unroll
        for (int j = 0; j < Q; ++j)
            forig[(size_t)chain * QP + j] = (unsigned char)(((j < 8 ? og_lo : og_hi) >> (4 * (j & 7))) & 15u);
    }
}

// ------------------------------------------------------------------ backward scan: state at every chunk end
__global__ void k_vit_scan_bwd(const unsigned char *__restrict__ forig, const int *__restrict__ sfinal,
                               int *__restrict__ send, Plan p) {
    const int seq = blockIdx.x * blockDim.x + threadIdx.x;
    if (seq >= p.NB) return;
    const size_t chain0 = (size_t)seq * p.C;
    int s = sfinal[seq];
    for (int c = p.C - 1; c >= 0; --c) {
        send[chain0 + c] = s;
        if (c > 0) s = forig[(chain0 + c) * QP + s];
    }
}

// ---- two-level backward scan: the maps "state at chunk end -> state before the chunk" compose exactly.
// k_vit_bwd_compose: per (sequence, group) the map of the whole group; k_vit_scan_bwd over the groups gives
// the state at every group's end; k_vit_bwd_inner walks the chunks of every group in parallel.
// SLAB (hmm_seqshard_viterbi.inc): the groups are whole time slabs, whose chunk 0 has a map of its own unless the slab
// starts its sequence; entries that mean nothing (states from q on, a slab that starts its sequence) leave as 0
template <bool SLAB>
__global__ void k_vit_bwd_compose(const unsigned char *__restrict__ forig, unsigned char *__restrict__ gforig, Plan p) {
    const long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x;       // (sequence, group, end state)
    if (id >= (long long)p.NB * p.G * QP) return;
    const int j = (int)(id & (QP - 1));
    const long long wv = id >> 4;
    const int seq = (int)(wv / p.G), grp = (int)(wv - (long long)seq * p.G);
    const int c0 = grp * p.gsize, c1 = min(p.C, c0 + p.gsize);
    int s = j;
    for (int c = c1 - 1; c >= c0; --c) s = forig[((size_t)seq * p.C + c) * QP + s] & 15;    // (hmm_viterbi never uses chunk 0's map)
    if (SLAB && (j >= p.q || p.seq_start)) s = 0;
    gforig[(size_t)wv * QP + j] = (unsigned char)s;
}

__global__ void k_vit_bwd_inner(const unsigned char *__restrict__ forig, const int *__restrict__ gsend,
                                int *__restrict__ send, Plan p) {
    const long long wv = (long long)blockIdx.x * blockDim.x + threadIdx.x;       // (sequence, group)
    if (wv >= (long long)p.NB * p.G) return;
    const int seq = (int)(wv / p.G), grp = (int)(wv - (long long)seq * p.G);
    const int c0 = grp * p.gsize, c1 = min(p.C, c0 + p.gsize);
    const size_t chain0 = (size_t)seq * p.C;
    int s = gsend[wv];                              // state at the end of the group's last chunk
    for (int c = c1 - 1; c >= c0; --c) {
        send[chain0 + c] = s;
        if (c > c0) s = forig[(chain0 + c) * QP + s];
    }
}

// ------------------------------------------------------------------ backtrace inside every chunk
#define VB_TS 16          // steps per staged backpointer tile: 16 words = 128 contiguous bytes per chain

// Lane = chain walks its chunk backwards.  The backpointer words of a wave's 64 chains for one step are
// 512 contiguous bytes (vit_bp_index), so every lane simply loads its own word — VB_TS steps ahead of the
// walk, which does not depend on them being followed.  Path entries are collected 64 steps x 64 chains in
// LDS and leave as 256-byte runs per chain.
__global__ __launch_bounds__(64) void k_vit_backtrace(const unsigned long long *__restrict__ bp, const int *__restrict__ send,
                                                      int *__restrict__ path, Plan p) {
    __shared__ unsigned char stage[64][64 + 4];           // [chain in wave][step in block]
    __shared__ long long cbase[64];                       // path index of every chain's chunk start
    __shared__ int clen[64];
    const int lane = threadIdx.x;
    const long long wchain0 = (long long)blockIdx.x * 64;
    const long long chain = wchain0 + lane;
    const bool inrange = chain < p.nchains;
    const long long chn = inrange ? chain : wchain0;
    const long long seq = chn / p.C;
    const int c = (int)(chn - seq * p.C);
    const int t0 = c * p.T;
    const int len = inrange ? min(p.T, p.L - t0) : 0;
    cbase[lane] = seq * p.L + t0;
    clen[lane] = len;
    int s = inrange ? send[chn] : 0;
    const unsigned long long *bpc = bp + vit_bp_index(wchain0 + lane, 0, p.T);      // step t: + t * 64
    __syncthreads();
    const int nblk = p.T / 64 + ((p.T % 64) ? 1 : 0);
    unsigned long long nx[VB_TS];
    auto fetch = [&](int ts) {                            // words of steps ts .. ts + VB_TS - 1
#pragma unroll
        for (int u = 0; u < VB_TS; ++u) nx[u] = (ts + u < len) ? bpc[(size_t)(ts + u) * 64] : 0ull;
    };
    // tiles are visited from the chunk's end; (blk, tl) -> first step blk * 64 + tl * VB_TS
    int ts_next = (nblk - 1) * 64 + (64 / VB_TS - 1) * VB_TS;
    while (ts_next >= p.T) ts_next -= VB_TS;
    fetch(ts_next);
    for (int blk = nblk - 1; blk >= 0; --blk) {
        for (int tl = 64 / VB_TS - 1; tl >= 0; --tl) {
            const int ts = blk * 64 + tl * VB_TS;         // first step of the tile (chunk-relative)
            if (ts >= p.T) continue;
            unsigned long long w[VB_TS];
#pragma unroll
            for (int u = 0; u < VB_TS; ++u) w[u] = nx[u];
            if (ts - VB_TS >= 0) fetch(ts - VB_TS);
#pragma unroll
            for (int u = VB_TS - 1; u >= 0; --u) {
                const int t = ts + u;
                if (t < len) {
                    stage[lane][tl * VB_TS + u] = (unsigned char)s;
                    if (t > 0) s = (int)((w[u] >> (4 * s)) & 15ull);
                }
            }
        }
        __syncthreads();
        // flush: 64 consecutive steps of one chain per store instruction
        for (int ch = 0; ch < 64; ++ch) {
            const int t = blk * 64 + lane;
#if HMM_VIT_NT
            if (t < clen[ch]) __builtin_nontemporal_store(stage[ch][lane], &path[cbase[ch] + t]);
#else
            if (t < clen[ch]) path[cbase[ch] + t] = stage[ch][lane];
#endif
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------ host entry
// ------------------------------------------------------------------ Viterbi, 16 < q <= 64
// Same Q16 integer semantics as hmm_viterbi.inc / oracle/viterbi.py:
//   d_t[j] = max_i (d_{t-1}[i] + Q(logA[i][j])) + Q(logE_t[j]),  lowest-index tie-breaks.
// One wave per sequence, lane = state: all q candidates are visited in increasing source index
// with strict '>', scores stay relative to the per-step maximum (int32) with an int64 base, one
// backpointer BYTE per (position, state) in 64-byte rows.  The backtrace runs in the same wave:
// 64 backpointer rows at a time are staged in LDS by all lanes, lane 0 walks them, and the 64 path
// entries leave coalesced.
#define MQ_NEG (-0x40000000)

__device__ __forceinline__ int mq_wave_max_i(int v) {
    v = row_max_i(v);
    float a = __builtin_bit_cast(float, v), bq = a;
    swap16(a, bq);
    v = max(__builtin_bit_cast(int, a), __builtin_bit_cast(int, bq));
    a = __builtin_bit_cast(float, v); bq = a;
    swap32(a, bq);
    return max(__builtin_bit_cast(int, a), __builtin_bit_cast(int, bq));
}

// the same maximum as a wave-uniform SCALAR, for rows 0 .. NR-1 of 16 lanes: four DPP stages with the shuffle as an
// operand modifier (one VALU instruction each; the intrinsic form costs a copy, a v_mov_dpp and the max), then one
// v_readlane per row and scalar maxima
template <int NR>
__device__ __forceinline__ int mq_wave_max_s(int v) {
    int a, b, c, d;
    asm("s_nop 1\n\tv_max_i32_dpp %0, %1, %1 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf" : "=&v"(a) : "v"(v));
    asm("s_nop 1\n\tv_max_i32_dpp %0, %1, %1 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf" : "=&v"(b) : "v"(a));
    asm("s_nop 1\n\tv_max_i32_dpp %0, %1, %1 row_half_mirror row_mask:0xf bank_mask:0xf" : "=&v"(c) : "v"(b));
    asm("s_nop 1\n\tv_max_i32_dpp %0, %1, %1 row_mirror row_mask:0xf bank_mask:0xf" : "=&v"(d) : "v"(c));
    int m = __builtin_amdgcn_readlane(d, 0);
#pragma unroll
    for (int r = 1; r < NR; ++r) m = max(m, __builtin_amdgcn_readlane(d, 16 * r));
    return m;
}

// the backtrace of one sequence, in the wave that filled its backpointer rows: 64 rows at a time are staged in
// LDS by all lanes (the next 64 are fetched into registers meanwhile: their memory latency, a third of the pass, is
// spent under the walk) and the 64 path entries leave coalesced.  Walking a block is a chain of dependent LDS
// reads, ~100 cycles each, on one lane; the maps compose, so all 64 lanes first form the 32 two-step, 16 four-step
// and 8 eight-step maps of the block (P1[l] = M_{2l+1} o M_{2l}, P2[l] = P1[2l+1] o P1[2l], P3 likewise: a read and a write
// per entry and level, no dependence between entries), lane 0 walks 8 eight-step hops, and the states in between come
// out of P2, P1 and M in three parallel rounds: 4.0 -> ~2.4 ms of the pass at L = 1e5.  (M_l[x] = rows[l][x]: the state at position
// tb - l - 1 of the path through state x at position tb - l.)  The sequence's first, partial block is walked row by row.
struct MqBtLds {
    unsigned char rows[64][64];
    unsigned char p1[32][64];
    unsigned char p2[16][64];
    unsigned char p3[8][64];
    int pbuf[64];
};
__device__ __forceinline__ void mq_backtrace(const unsigned char *bpr, int *pr, int L, int j, int s, MqBtLds &lds) {
    i4 nx[4];
    auto fetch = [&](int t) {
        if (t >= 1) {
            const i4 *src = reinterpret_cast<const i4 *>(bpr + (size_t)t * 64);
            nx[0] = src[0]; nx[1] = src[1]; nx[2] = src[2]; nx[3] = src[3];
        }
    };
    fetch(L - 1 - j);
    for (int tb = L - 1; tb >= 0; tb -= 64) {
        const int t = tb - j;
        if (t >= 1) {
            i4 *dst = reinterpret_cast<i4 *>(&lds.rows[j][0]);
            dst[0] = nx[0]; dst[1] = nx[1]; dst[2] = nx[2]; dst[3] = nx[3];
        }
        fetch(t - 64);
        __syncthreads();
        if (tb - 63 >= 1) {                                  // a whole block: every row is a real backpointer row
            // (all reads of a round before any write: byte stores may alias everything, the compiler would
            // otherwise run the entries one after the other)
            unsigned a[32];
#pragma unroll
            for (int l = 0; l < 32; ++l) a[l] = lds.rows[2 * l][j];
#pragma unroll
            for (int l = 0; l < 32; ++l) a[l] = lds.rows[2 * l + 1][a[l] & 63];
#pragma unroll
            for (int l = 0; l < 32; ++l) lds.p1[l][j] = (unsigned char)a[l];
            // the lane's own column of P1 is enough for its column of P2's first factor; the second is anybody's
            __syncthreads();
#pragma unroll
            for (int l = 0; l < 16; ++l) a[l] = lds.p1[2 * l + 1][a[2 * l] & 63];
#pragma unroll
            for (int l = 0; l < 16; ++l) lds.p2[l][j] = (unsigned char)a[l];
            __syncthreads();
#pragma unroll
            for (int l = 0; l < 8; ++l) a[l] = lds.p2[2 * l + 1][a[2 * l] & 63];
#pragma unroll
            for (int l = 0; l < 8; ++l) lds.p3[l][j] = (unsigned char)a[l];
            __syncthreads();
            if (j == 0) {
                int v = s;
#pragma unroll
                for (int l = 0; l < 8; ++l) {
                    lds.pbuf[8 * l] = v;
                    v = lds.p3[l][v & 63];                   // eight positions down the path
                }
                s = v;
            }
            __syncthreads();
            if (j < 8) lds.pbuf[8 * j + 4] = lds.p2[2 * j][lds.pbuf[8 * j] & 63];
            __syncthreads();
            if (j < 16) lds.pbuf[4 * j + 2] = lds.p1[2 * j][lds.pbuf[4 * j] & 63];
            __syncthreads();
            if (j < 32) lds.pbuf[2 * j + 1] = lds.rows[2 * j][lds.pbuf[2 * j] & 63];
        } else if (j == 0) {
            for (int l = 0; l < 64 && tb - l >= 0; ++l) {
                lds.pbuf[l] = s;
                if (tb - l >= 1) s = lds.rows[l][s & 63];    // predecessor of state s at position tb - l
            }
        }
        __syncthreads();
        if (t >= 0) pr[t] = lds.pbuf[j];
        s = __builtin_amdgcn_readfirstlane(s);               // lane 0 walked: its state continues the path
        __syncthreads();
    }
}

// SPARSE models (the gene models of 29 / 43 / 57 states have at most 3 / 4 / 5 edges into a state): lane j visits
// its own predecessors only — D ds_bpermute gathers instead of q readlane broadcasts — and every entry equal to the
// matrix minimum ("log zero") is covered by ONE candidate, the previous step's best state plus that minimum
// (k_vit_prep's rule, exact: a state that is an explicit predecessor beats its own off-edge candidate strictly,
// and among the others the best state dominates).  Lowest-index tie-breaks as in the all-candidates loop:
// explicit predecessors in increasing index with strict '>', the off-edge candidate wins a tie only with a lower
// index.  k_mq_prep decides per model on the device.
#define MQ_DMAX 8
struct MqModel {
    int mode;                 // 0: all-candidates loop (a state with more than MQ_DMAX explicit predecessors); else D: 3, 4 or 8
    int a_off;                // matrix minimum
    int src[64][MQ_DMAX];     // explicit predecessors of state j, increasing; pads: j itself with weight MQ_NEG
    int wgt[64][MQ_DMAX];
};

__global__ __launch_bounds__(64) void k_mq_prep(const float *__restrict__ logA, MqModel *__restrict__ models, int q,
                                                int force_dense) {
    const int m = blockIdx.x, j = threadIdx.x;
    const float *Am = logA + (size_t)m * q * q;
    const bool act = j < q;
    int amin = 0x7fffffff;
    for (int i = 0; i < q; ++i) amin = act ? min(amin, vquant(Am[(size_t)i * q + j])) : amin;
    amin = -mq_wave_max_i(-amin);
    MqModel &M = models[m];
    int n = 0;
    for (int i = 0; i < q; ++i) {
        const int v = act ? vquant(Am[(size_t)i * q + j]) : amin;
        if (v > amin) {
            if (n < MQ_DMAX) { M.src[j][n] = i; M.wgt[j][n] = v; }
            ++n;
        }
    }
    for (int e = n; e < MQ_DMAX; ++e) { M.src[j][e] = j; M.wgt[j][e] = MQ_NEG; }
    const int deg = mq_wave_max_i(n);
    if (j == 0) {
        M.mode = (force_dense || deg > MQ_DMAX) ? 0 : (deg <= 3 ? 3 : (deg <= 4 ? 4 : 8));
        M.a_off = amin;
    }
}

// cand[i] = d[lane i] + acol[i] for i = 0 .. QB-1 (the all-candidates step)
template <int QB, int I> struct MqCand {
    static __device__ __forceinline__ void fill(int d, int lane, const int (&acol)[QB], int (&cand)[QB]) {
        int dr[QB / 16];
#pragma unroll
        for (int r = 0; r < QB / 16; ++r) dr[r] = __builtin_amdgcn_ds_bpermute((16 * r + (lane & 15)) * 4, d);
        step<0>(dr, acol, cand);
    }
    template <int K> static __device__ __forceinline__ void step(const int (&dr)[QB / 16], const int (&acol)[QB], int (&cand)[QB]) {
        if constexpr (K < QB) {
            if (K % 16 == 0)
                asm volatile("s_nop 1\n\tv_add_u32_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf" : "=v"(cand[K]) : "v"(dr[K / 16]), "v"(acol[K]), "n"(K % 16));
            else
                asm volatile("v_add_u32_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf" : "=v"(cand[K]) : "v"(dr[K / 16]), "v"(acol[K]), "n"(K % 16));
            step<K + 1>(dr, acol, cand);
        }
    }
};

// D = 0: all q candidates per step (column j of Q(logA) in QB registers); D = 4 / 8: the sparse step.
// The emission rows arrive through raw buffer loads MQ_PF steps ahead with no branch around them (rows past the
// sequence are outside the descriptor and read 0): with the loads under `if (t + MQ_PF < L)` the compiler waited
// for vmcnt(0) every step — a full memory latency, 0.55 of the 0.6 us per step.
template <int QB, int D>
__global__ __launch_bounds__(64) void k_mq_viterbi(const MqModel *__restrict__ models,
                                                   const float *__restrict__ logA, const float *__restrict__ logpi,
                                                   const float *__restrict__ logE, int b, int L, int q,
                                                   unsigned char *__restrict__ bp, int *__restrict__ path,
                                                   double *__restrict__ score) {
    __shared__ __attribute__((aligned(16))) MqBtLds btl;
    const int row = blockIdx.x, m = row / b, j = threadIdx.x;
    const MqModel &M = models[m];
    if (M.mode != D) return;                                // the other instantiation has this model
    const bool act = j < q;
    constexpr int NA = D ? 1 : QB;
    int acol[NA];
    // predecessors and weights as vector VALUES (a register array of them indexed by the selects below ends up
    // in scratch: the compiler turns "select of array elements" into "array element at a selected index")
    i4 sa = {0, 0, 0, 0}, sb = sa, wa = sa, wb = sa;
    if constexpr (D == 0) {
        const float *Am = logA + (size_t)m * q * q;
#pragma unroll
        for (int i = 0; i < QB; ++i) acol[i] = (act && i < q) ? vquant(Am[(size_t)i * q + j]) : 0;
    } else {
        sa = *reinterpret_cast<const i4 *>(&M.src[j][0]); wa = *reinterpret_cast<const i4 *>(&M.wgt[j][0]);
        if constexpr (D == 8) { sb = *reinterpret_cast<const i4 *>(&M.src[j][4]); wb = *reinterpret_cast<const i4 *>(&M.wgt[j][4]); }
    }
    auto pick = [](const i4 &a, const i4 &b, int x) {       // x is a constant after unrolling
        const i4 v = x < 4 ? a : b;
        return (x & 3) == 0 ? v.x : ((x & 3) == 1 ? v.y : ((x & 3) == 2 ? v.z : v.w));
    };
    const int a_off = M.a_off;
    const float *Er = logE + (size_t)row * L * q;
    unsigned char *bpr = bp + (size_t)row * L * 64;
    const int rowb = q * (int)sizeof(float);
    const int voff = act ? j * 4 : 0;                       // (idle lanes read state 0's value and ignore it)
    auto rows_from = [&](long long t0) {                    // descriptor of rows t0 .. L-1 of this sequence
        const long long rem = ((long long)L - t0) * rowb;
        return make_rsrc(Er + t0 * q, rem > 0 ? (unsigned long long)(rem < (1ll << 20) ? rem : (1ll << 20)) : 0ull);
    };
    // d: the scores of the previous step relative to `base`.  Sparse step: base LAGS one step — it advances by the
    // maximum of d_{t-1} while step t's gathers are in flight — so the wave-wide maximum (and the lowest index
    // that attains it: the off-edge candidate) is off the step's dependent chain, which is gather, add, max3,
    // max3, add.  Integer arithmetic: the frame a score is expressed in changes nothing; d stays within
    // [-2^29, 2^27].
    constexpr int NR = QB / 16;
    int d;
    long long base = 0;
    {
        const float e0 = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rows_from(0), voff, 0, 0));
        d = act ? vquant(logpi[(size_t)m * q + j]) + vquant(e0) : MQ_NEG;
#ifndef MQ_X_NOSTORE
        bpr[j] = (unsigned char)j;
#endif
    }
    auto step = [&](int t, float ef) {
        if constexpr (D == 0) {
            const int e = vquant(ef);
            // every candidate in ONE instruction (each 16-lane row of d replicated into every row by a ds_bpermute,
            // then v_add_u32 with the DPP row broadcast as its operand modifier), the maximum first — a chain of QB / 2
            // v_max3 instead of QB compare-and-select pairs — and who achieved it afterwards, every compare
            // independent: the lowest index among the maxima, as the strict '>' in increasing order gave
            int cand[QB];
            MqCand<QB, 0>::fill(d, j, acol, cand);                               // lanes >= q hold MQ_NEG: never win
            int best = cand[0];
#pragma unroll
            for (int i = 1; i + 1 < QB; i += 2) best = max(max(best, cand[i]), cand[i + 1]);
            best = max(best, cand[QB - 1]);
            int arg = QB - 1;
#pragma unroll
            for (int i = QB - 2; i >= 0; --i) arg = cand[i] == best ? i : arg;
            const int y = act ? best + e : MQ_NEG;         // (q dependent broadcasts: nothing gained by lagging)
            const int mx = mq_wave_max_i(y);
            base += mx;
            d = act ? y - mx : MQ_NEG;
#ifndef MQ_X_NOSTORE
            bpr[(size_t)t * 64 + j] = (unsigned char)arg;
#endif
        } else {
            // the score first (it alone feeds the next step), then who achieved it: the lowest index among the
            // explicit predecessors that reach it (they are stored in increasing order) and, if the off-edge
            // candidate — every non-edge at once: the best previous state, lowest index istar, plus a_off —
            // reaches it too, the lower of the two.  (Pinning the order by hand with sched_barrier — gathers, then
            // the previous step's backpointers and this step's maximum under them, then the chain — was slower
            // than the compiler's own interleaving, 19.1 against 17.6 ms: the wave is issue-bound.)
            int cand[D];
#pragma unroll
            for (int x = 0; x < D; ++x) cand[x] = __builtin_amdgcn_ds_bpermute(pick(sa, sb, x) * 4, d);
            const int mx = mq_wave_max_s<NR>(d);
            const int istar = __builtin_ctzll(__builtin_amdgcn_ballot_w64(d == mx));
            const int off = mx + a_off;
            const int em = vquant(ef) - mx;
            base += mx;
#pragma unroll
            for (int x = 0; x < D; ++x) cand[x] += pick(wa, wb, x);
            int best = off;
#pragma unroll
            for (int x = 0; x < D; ++x) best = max(best, cand[x]);
            d = act ? best + em : MQ_NEG;
            int arg = 64;
#pragma unroll
            for (int x = D - 1; x >= 0; --x) arg = cand[x] == best ? pick(sa, sb, x) : arg;
            arg = off == best ? min(arg, istar) : arg;
#ifndef MQ_X_NOSTORE
            bpr[(size_t)t * 64 + j] = (unsigned char)arg;
#endif
        }
    };
    float en[MQ_PF];
    {
        const __amdgpu_buffer_rsrc_t rs = rows_from(1);
#pragma unroll
        for (int u = 0; u < MQ_PF; ++u)
            en[u] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, voff + u * rowb, 0, 0));
    }
    // Nothing in flight when the loop is entered: the compiler's wait counts at the loop head are the more
    // cautious of the two ways in, and coming from here the rows just requested have only the first backpointer
    // store behind them — it would then wait, every block, until all but one of the block's STORES have been
    // acknowledged as well (vmcnt counts both on gfx9).
    __builtin_amdgcn_s_waitcnt(0x0F70);                     // vmcnt(0)
    int tb = 1;
    for (; tb + MQ_PF <= L; tb += MQ_PF) {                  // whole blocks: no branch inside
        const __amdgpu_buffer_rsrc_t rs = rows_from((long long)tb + MQ_PF);
#pragma unroll
        for (int u = 0; u < MQ_PF; ++u) {
            const float ef = en[u];
            en[u] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, voff + u * rowb, 0, 0));
            step(tb + u, ef);
        }
    }
#pragma unroll
    for (int u = 0; u < MQ_PF; ++u)
        if (tb + u < L) step(tb + u, en[u]);                // wave-uniform
    const int mxl = mq_wave_max_s<NR>(d);
    const int istar = __builtin_ctzll(__builtin_amdgcn_ballot_w64(d == mxl));     // lowest index among the best
    base += mxl;
    if (j == 0) score[row] = (double)base / (double)VQ_SCALE;
#ifndef MQ_X_NOBT
    mq_backtrace(bpr, path + (size_t)row * L, L, j, istar, btl);
#endif
}

static size_t mq_viterbi_workspace(int k, int b, int L) {
    return align_up((size_t)k * b * L * 64) + align_up((size_t)k * sizeof(MqModel));
}

static void mq_viterbi(const float *logA, const float *logpi, const float *logE, int k, int b, int L, int q,
                       unsigned char *bp, int *path, double *score, hipStream_t st) {
    const dim3 grid((unsigned)(k * b));
    MqModel *models = (MqModel *)(bp + align_up((size_t)k * b * L * 64));
    hipLaunchKernelGGL(k_mq_prep, dim3(k), dim3(64), 0, st, logA, models, q, opt(HMM_OPT_FORCE_DENSE) == 1 ? 1 : 0);
    const MqModel *cm = models;
    if (q <= 32) {
        hipLaunchKernelGGL((k_mq_viterbi<32, 3>), grid, dim3(64), 0, st, cm, logA, logpi, logE, b, L, q, bp, path, score);
        hipLaunchKernelGGL((k_mq_viterbi<32, 4>), grid, dim3(64), 0, st, cm, logA, logpi, logE, b, L, q, bp, path, score);
        hipLaunchKernelGGL((k_mq_viterbi<32, 8>), grid, dim3(64), 0, st, cm, logA, logpi, logE, b, L, q, bp, path, score);
        hipLaunchKernelGGL((k_mq_viterbi<32, 0>), grid, dim3(64), 0, st, cm, logA, logpi, logE, b, L, q, bp, path, score);
    } else {
        hipLaunchKernelGGL((k_mq_viterbi<64, 3>), grid, dim3(64), 0, st, cm, logA, logpi, logE, b, L, q, bp, path, score);
        hipLaunchKernelGGL((k_mq_viterbi<64, 4>), grid, dim3(64), 0, st, cm, logA, logpi, logE, b, L, q, bp, path, score);
        hipLaunchKernelGGL((k_mq_viterbi<64, 8>), grid, dim3(64), 0, st, cm, logA, logpi, logE, b, L, q, bp, path, score);
        if (q <= 48)
            hipLaunchKernelGGL((k_mq_viterbi<48, 0>), grid, dim3(64), 0, st, cm, logA, logpi, logE, b, L, q, bp, path, score);
        else
            hipLaunchKernelGGL((k_mq_viterbi<64, 0>), grid, dim3(64), 0, st, cm, logA, logpi, logE, b, L, q, bp, path, score);
    }
}

extern "C" int hmm_viterbi_max_states(void) { return MQ_MAX; }

// ---- batch groups.  The chunk reduce is integer-VALU-bound (2.1 TB/s of emission reads), the in-chunk pass +
// backtrace are memory-side work that leaves the VALUs idle, and the whole job moves less than half of what
// HBM could deliver in its time.  A large batch is therefore cut into two groups of sequences, and reduce +
// scan of the second run on the caller's stream underneath apply + backtrace of the first on a helper stream.
// Two kernels only share a CU if the first leaves room: with the reduce at its natural 4 waves per SIMD
// nothing overlapped at all (5.15 ms with or without groups); held to 3 it is as fast and one wave per SIMD of
// the in-chunk pass fits beside it: 4.85 ms (2 waves: the reduce itself slows, 5.4; more groups: each kernel
// gets too small, 5.0-5.9) — tools/experiments/ab_vit.py, vit_time.py.  Groups are independent problems and
// integer max-plus is exact whatever the chunk length: identical paths and scores.
#define VIT_MAX_GROUPS 8
struct VGroups {
    int n, b0[VIT_MAX_GROUPS + 1];
    VPlan plan[VIT_MAX_GROUPS];
    size_t off[VIT_MAX_GROUPS], total;
};
static int vit_groups(int b, int L, int q, VGroups *G) {
    int n = opt(HMM_OPT_VGROUPS);
    if (n <= 0) n = ((long long)b * L >= (1ll << 26) && b >= 64) ? 2 : 1;       // auto: only while half the batch still fills the machine
    if (n > VIT_MAX_GROUPS) n = VIT_MAX_GROUPS;
    if (n > b / 16) n = b / 16 > 0 ? b / 16 : 1;
    G->n = n;
    size_t off = 0;
    for (int g = 0; g <= n; ++g) G->b0[g] = g == n ? b : (int)((long long)b * g / n / 16 * 16);
    for (int g = 0; g < n; ++g) {
        int rc = make_vplan(G->b0[g + 1] - G->b0[g], L, q, &G->plan[g]);
        if (rc) return rc;
        G->off[g] = off;
        off = align_up(off + G->plan[g].total);
    }
    G->total = off;
    return HMM_OK;
}

// the chunk operators of one model's chains (the kernel that does not serve the model returns at once)
static void vit_launch_reduce(const float *Em, const VPlan &v, char *ws, const VModel *model, int q, hipStream_t st) {
    const Plan &p = v.p;
    int *vops = (int *)(ws + v.o_vops);
    long long *vbase = (long long *)(ws + v.o_vbase);
    const unsigned nb16 = (unsigned)((p.nchains + 15) / 16);
    if (q == TopoGene15::Q)
        hipLaunchKernelGGL(k_vit_reduce_sparse<TopoGene15>, dim3(nb16), dim3(256), 0, st, Em, model, vops, vbase, p);
    else if (q == TopoGene7::Q)
        hipLaunchKernelGGL(k_vit_reduce_sparse<TopoGene7>, dim3(nb16), dim3(256), 0, st, Em, model, vops, vbase, p);
    hipLaunchKernelGGL(k_vit_reduce, dim3(nb16), dim3(256), 0, st, Em, model, vops, vbase, p);
}

// reduce + chunk scan of one group (scores -> score), on st
static void vit_phase_a(const float *Em, const VPlan &v, char *ws, const VModel *model, double *score, int q,
                        hipStream_t st) {
    const Plan &p = v.p;
    int *vops = (int *)(ws + v.o_vops);
    long long *vbase = (long long *)(ws + v.o_vbase);
    int *dstart = (int *)(ws + v.o_dstart);
    long long *dbase = (long long *)(ws + v.o_dbase);
    int *sfinal = (int *)(ws + v.o_sfinal);
    vit_launch_reduce(Em, v, ws, model, q, st);
    const bool two = p.G > 0 && opt(HMM_OPT_SCAN2) != 0;
    if (!two) {
        hipLaunchKernelGGL(k_vit_scan_fwd, dim3(p.NB), dim3(64), 0, st, (const int *)vops, (const long long *)vbase,
                           dstart, dbase, sfinal, score, p);
    } else {
        int *gvops = (int *)(ws + v.o_gvops), *gdstart = (int *)(ws + v.o_gdstart);
        long long *gvbase = (long long *)(ws + v.o_gvbase), *gdbase = (long long *)(ws + v.o_gdbase);
        const long long nwv = (long long)p.NB * p.G;
        hipLaunchKernelGGL(k_vit_scan_compose, dim3((unsigned)((nwv + 3) / 4)), dim3(256), 0, st, (const int *)vops,
                           (const long long *)vbase, gvops, gvbase, p);
        Plan pg = p;
        pg.C = p.G;
        hipLaunchKernelGGL(k_vit_scan_fwd, dim3(p.NB), dim3(64), 0, st, (const int *)gvops, (const long long *)gvbase,
                           gdstart, gdbase, sfinal, score, pg);
        hipLaunchKernelGGL(k_vit_scan_inner, dim3((unsigned)nwv), dim3(64), 0, st, (const int *)vops,
                           (const long long *)vbase, (const int *)gdstart, (const long long *)gdbase, dstart, dbase, p);
    }
}

// the in-chunk pass of one model's chains from the scores entering them: backpointers and the chunks' maps
static void vit_launch_apply(const float *Em, const VPlan &v, char *ws, const VModel *model, int q, hipStream_t st) {
    const Plan &p = v.p;
    const int *dstart = (const int *)(ws + v.o_dstart);
    unsigned char *forig = (unsigned char *)(ws + v.o_forig);
    unsigned long long *bp = (unsigned long long *)(ws + v.o_bp);
    const unsigned nb16 = (unsigned)((p.nchains + 15) / 16), nb64 = (unsigned)((p.nchains + 63) / 64);
    if (q == TopoGene15::Q)
        hipLaunchKernelGGL(k_vit_apply_sparse<TopoGene15>, dim3(nb64), dim3(64), 0, st, Em, model, dstart, forig, bp, p);
    else if (q == TopoGene7::Q)
        hipLaunchKernelGGL(k_vit_apply_sparse<TopoGene7>, dim3(nb64), dim3(64), 0, st, Em, model, dstart, forig, bp, p);
    hipLaunchKernelGGL(k_vit_apply, dim3(nb16), dim3(256), 0, st, Em, model, dstart, forig, (unsigned int *)bp, p);
}

// backward chunk scan from the sequences' end states (o_sfinal) and backtrace (-> path), on st; gforig_ready: the
// groups' maps are already in the workspace
static void vit_launch_backtrace(const VPlan &v, char *ws, int32_t *path, bool gforig_ready, hipStream_t st) {
    const Plan &p = v.p;
    unsigned char *forig = (unsigned char *)(ws + v.o_forig);
    int *send = (int *)(ws + v.o_send);
    const int *sfinal = (const int *)(ws + v.o_sfinal);
    unsigned long long *bp = (unsigned long long *)(ws + v.o_bp);
    const bool two = p.G > 0 && opt(HMM_OPT_SCAN2) != 0;
    if (!two) {
        hipLaunchKernelGGL(k_vit_scan_bwd, dim3((p.NB + 63) / 64), dim3(64), 0, st, (const unsigned char *)forig, sfinal,
                           send, p);
    } else {
        unsigned char *gforig = (unsigned char *)(ws + v.o_gforig);
        int *gsend = (int *)(ws + v.o_gsend);
        const long long nwv = (long long)p.NB * p.G;
        if (!gforig_ready)
            hipLaunchKernelGGL(k_vit_bwd_compose<false>, dim3((unsigned)((nwv * QP + 255) / 256)), dim3(256), 0, st,
                               (const unsigned char *)forig, gforig, p);
        Plan pg = p;
        pg.C = p.G;
        hipLaunchKernelGGL(k_vit_scan_bwd, dim3((p.NB + 63) / 64), dim3(64), 0, st, (const unsigned char *)gforig, sfinal,
                           gsend, pg);
        hipLaunchKernelGGL(k_vit_bwd_inner, dim3((unsigned)((nwv + 63) / 64)), dim3(64), 0, st,
                           (const unsigned char *)forig, (const int *)gsend, send, p);
    }
    hipLaunchKernelGGL(k_vit_backtrace, dim3((unsigned)((p.nchains + 63) / 64)), dim3(64), 0, st,
                       (const unsigned long long *)bp, (const int *)send, path, p);
}

// in-chunk pass, backward chunk scan and backtrace of one group (-> path), on st
static void vit_phase_b(const float *Em, const VPlan &v, char *ws, const VModel *model, int32_t *path, int q,
                        hipStream_t st) {
    vit_launch_apply(Em, v, ws, model, q, st);
    vit_launch_backtrace(v, ws, path, false, st);
}

extern "C" size_t hmm_viterbi_workspace_bytes(int k, int b, int L, int q) {
    if (q > QP && q <= MQ_MAX) return (k < 1 || b < 1 || L < 1) ? 0 : mq_viterbi_workspace(k, b, L);
    VGroups G;
    if (k < 1 || b < 1 || vit_groups(b, L, q, &G)) return 0;
    return G.total;
}

extern "C" int hmm_viterbi(const float *logA, const float *logpi, const float *logE, int k, int b, int L, int q,
                           int32_t *path, double *score, void *workspace, size_t workspace_bytes, void *stream) {
    if (k < 1) return HMM_ERR_BAD_SHAPE;
    if (q > QP && q <= MQ_MAX) {                             // one wave per sequence (hmm_midq.inc)
        if (b < 1 || L < 1) return HMM_ERR_BAD_SHAPE;
        if (!logA || !logpi || !logE || !path || !score || !workspace) return HMM_ERR_NULL_POINTER;
        if (workspace_bytes < mq_viterbi_workspace(k, b, L) || ((uintptr_t)workspace & 255)) return HMM_ERR_WORKSPACE;
        mq_viterbi(logA, logpi, logE, k, b, L, q, (unsigned char *)workspace, path, score, (hipStream_t)stream);
        return check_launch();
    }
    if (b < 1) return HMM_ERR_BAD_SHAPE;
    VGroups G;
    int rc = vit_groups(b, L, q, &G);
    if (rc) return rc;
    if (!logA || !logpi || !logE || !path || !score || !workspace) return HMM_ERR_NULL_POINTER;
    if (workspace_bytes < G.total || ((uintptr_t)workspace & 255)) return HMM_ERR_WORKSPACE;
    char *ws = (char *)workspace;
    hipStream_t st = (hipStream_t)stream;
    hipStream_t *hs = G.n > 1 ? helper_streams() : nullptr;
    hipStream_t side = hs ? hs[0] : st;                      // no helper stream: everything in order on st
    VModel *model = (VModel *)(ws + G.off[0] + G.plan[0].o_model);
    const int force_generic = opt(HMM_OPT_FORCE_DENSE) == 1 ? 1 : 0;
    // one model at a time (the workspace is reused), so the blocks of the lane-per-(chain, x) kernels never
    // mix models
    for (int m = 0; m < k; ++m) {
        hipLaunchKernelGGL(k_vit_prep, dim3(1), dim3(64), 0, st, logA + (size_t)m * q * q, logpi + (size_t)m * q, model, q,
                           force_generic);
        hipEvent_t ev;
        for (int g = 0; g < G.n; ++g) {
            const size_t r0 = (size_t)m * b + G.b0[g];
            const float *Em = logE + r0 * L * q;
            vit_phase_a(Em, G.plan[g], ws + G.off[g], model, score + r0, q, st);
            if (side != st) {
                (void)hipEventCreateWithFlags(&ev, hipEventDisableTiming);
                (void)hipEventRecord(ev, st);
                (void)hipStreamWaitEvent(side, ev, 0);
                (void)hipEventDestroy(ev);
            }
            vit_phase_b(Em, G.plan[g], ws + G.off[g], model, path + r0 * L, q, side);
        }
        if (side != st) {                                    // join (also before the next model reuses the workspace)
            (void)hipEventCreateWithFlags(&ev, hipEventDisableTiming);
            (void)hipEventRecord(ev, side);
            (void)hipStreamWaitEvent(st, ev, 0);
            (void)hipEventDestroy(ev);
        }
    }
    return check_launch();
}
