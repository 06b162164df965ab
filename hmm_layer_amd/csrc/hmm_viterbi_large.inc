// hmm_viterbi_large.inc — Viterbi for 1 <= q <= 4096 states (hmm_viterbi_large), included after hmm_viterbi.inc.
//
// Same Q16 semantics as hmm_viterbi.inc / oracle/viterbi.py:
//   Q(x) = rint(clip(x, -1024, 1024) * 65536),  d_t[j] = max_i (d_{t-1}[i] + Q(logA[i][j])) + Q(logE_t[j]),
// lowest-index tie-breaks in the recursion and at the final state, score = integer / 2^16.  Every evaluation
// below visits candidates so that the lowest maximising index wins, and integer max-plus is exact in any
// order: paths and scores are bit-identical to the serial recursion.
//
// No saturation (both paths).  Every Q term lies in [-2^26, 2^26].  Let M_t = max_j d_t[j].  State j is
// reachable from the previous best state at cost Q(logA[i*][j]) + Q(logE_t[j]) >= -2^27, and no step adds more
// than 2^27, so M_{t-1} - 2^27 <= d_t[j] <= M_{t-1} + 2^27 for EVERY j.  Scores are kept as int32 relative to
// the previous step's maximum (a running 64-bit base per sequence carries the frame): every stored value lies in
// [-2^28, 2^27] and every candidate formed from it in [-2^28 - 2^26, 2^27 + 2^26].
//
// Kernels:
//   k_vl_prep     per model: Q(logpi), the matrix minimum a_off and maximum a_max, and (q <= VL_WALK_MAX) the
//                 explicit edges of every destination — entries above a_off, increasing source — with the
//                 largest in-degree, which picks the walk's step (sparse D = 4 / 8, or all candidates).
//   k_vl_walk     per-sequence walk (HMM_OPT_VLARGE = 1): one workgroup per sequence, lane = state, the
//                 previous vector double-buffered in LDS with one barrier per step; the backtrace in the same
//                 workgroup from backpointer rows staged in LDS.
//   k_vl_init / k_vl_tile / k_vl_final   per-position tiles (HMM_OPT_VLARGE = 2): one launch per position over
//                 the whole batch, rows = sequences, columns = destinations, K = sources, integer max-plus with
//                 packed argmax keys; k_vl_final takes the last maximum and walks the backpointers, one lane
//                 per sequence.
// Backpointers are uint16 at ((row * L) + t) * q + j, 64-bit offsets throughout.

#define VL_MAX 4096               // hmm_viterbi_large_max_states()
#define VL_WALK_MAX 1024          // largest q the walk serves (one workgroup of up to 1024 lanes)
#define VL_Q_WALK 128             // default route: walk for q <= VL_Q_WALK, tiles above
#define VL_DMAX 8                 // explicit predecessors a sparse walk step visits
#define VL_NEG (-0x40000000)      // below every stored score (>= -2^28)
#define VL_KEY_MIN (-0x7fffffff - 1)
#define VL_DENSE_LDS 128          // dense walk: Q(log A) staged in LDS for q <= this (64 KB)

struct VlModel {
    int mode;        // walk step: 0 all candidates, 4 or 8 explicit predecessors + the covering candidate
    int a_off;       // matrix minimum: value of every entry that is not an explicit edge
    int a_max;       // matrix maximum (tile keys are formed relative to it)
    int deg;         // largest explicit in-degree
};

struct VlLayout {
    size_t o_bp, o_model, o_p0, o_src, o_wgt, o_P, o_pm, o_base, total;
    int ncolt;       // column tiles of the tile path
};

#define VL_BM 64                  // tile: rows (sequences)
#define VL_BN 64                  //       columns (destination states)
#define VL_BK 16                  //       sources per LDS slab = per packed-key slab (4 index bits)

static void vl_layout(int k, int b, int L, int q, VlLayout *v) {
    const size_t nr = (size_t)k * b;
    const int qw = q < VL_WALK_MAX ? q : VL_WALK_MAX;
    v->ncolt = (q + VL_BN - 1) / VL_BN;
    size_t off = 0;
    v->o_bp = off;    off = align_up(off + nr * L * q * sizeof(unsigned short));
    v->o_model = off; off = align_up(off + (size_t)k * sizeof(VlModel));
    v->o_p0 = off;    off = align_up(off + (size_t)k * q * sizeof(int));
    v->o_src = off;   off = align_up(off + (size_t)k * qw * VL_DMAX * sizeof(int));
    v->o_wgt = off;   off = align_up(off + (size_t)k * qw * VL_DMAX * sizeof(int));
    v->o_P = off;     off = align_up(off + 2 * nr * q * sizeof(int));
    v->o_pm = off;    off = align_up(off + 2 * nr * v->ncolt * sizeof(int));
    v->o_base = off;  off = align_up(off + nr * sizeof(long long));
    v->total = off;
}

__device__ __forceinline__ int vl_wave_min(int v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = min(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ int vl_wave_max(int v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = max(v, __shfl_xor(v, o));
    return v;
}

// grid k, block 1024: the matrix extremes in one coalesced pass over the model; the edge lists (walk only) per column
__global__ __launch_bounds__(1024) void k_vl_prep(const float *__restrict__ logA, const float *__restrict__ logpi,
                                                  VlModel *__restrict__ models, int *__restrict__ p0,
                                                  int *__restrict__ src, int *__restrict__ wgt, int q, int edges,
                                                  int force_dense) {
    __shared__ int red[3][16];
    const int m = blockIdx.x, tid = threadIdx.x, w = tid >> 6;
    const float *Am = logA + (size_t)m * q * q;
    int lo = 0x7fffffff, hi = -0x7fffffff;
    const size_t nq = (size_t)q * q;
#pragma unroll 8
    for (size_t x = tid; x < nq; x += 1024) {
        const int v = vquant(Am[x]);
        lo = min(lo, v);
        hi = max(hi, v);
    }
    for (int j = tid; j < q; j += 1024) p0[(size_t)m * q + j] = vquant(logpi[(size_t)m * q + j]);
    lo = vl_wave_min(lo);
    hi = vl_wave_max(hi);
    if ((tid & 63) == 0) { red[0][w] = lo; red[1][w] = hi; }
    __syncthreads();
    lo = red[0][0]; hi = red[1][0];
    for (int x = 1; x < 16; ++x) { lo = min(lo, red[0][x]); hi = max(hi, red[1][x]); }
    int deg = 0;
    if (edges && q <= VL_WALK_MAX && tid < q) {
        const int j = tid;
        int *sj = src + ((size_t)m * q + j) * VL_DMAX, *wj = wgt + ((size_t)m * q + j) * VL_DMAX;
        int n = 0;
        for (int i = 0; i < q; ++i) {
            const int v = vquant(Am[(size_t)i * q + j]);
            if (v > lo) {
                if (n < VL_DMAX) { sj[n] = i; wj[n] = v; }
                ++n;
            }
        }
        for (int e = n; e < VL_DMAX; ++e) { sj[e] = j; wj[e] = VL_NEG; }     // pads: never win
        deg = n;
    }
    deg = vl_wave_max(deg);
    if ((tid & 63) == 0) red[2][w] = deg;
    __syncthreads();
    if (tid == 0) {
        for (int x = 1; x < 16; ++x) deg = max(deg, red[2][x]);
        VlModel &M = models[m];
        M.a_off = lo;
        M.a_max = hi;
        M.deg = deg;
        M.mode = (force_dense || !edges || q > VL_WALK_MAX || deg > VL_DMAX) ? 0 : (deg <= 4 ? 4 : 8);
    }
}

// ------------------------------------------------------------------ per-sequence walk
// D = 4 / 8: lane j visits its explicit predecessors (increasing, strict '>') and the covering candidate — the
// previous step's best state i* (lowest index) plus a_off, which stands for every absent edge at once: an explicit
// predecessor beats its own off-edge value, and among the others i* dominates; the covering candidate wins a tie
// only with a lower index (hmm_viterbi.inc, k_mq_prep).  D = 0: every source in increasing order, strict '>'.
// The previous step's maximum and i* come from per-wave partials written before the step's barrier.
struct VlWalkLds {
    int d[2][VL_WALK_MAX];
    int wmx[2][16];
    int warg[2][16];
    int pbuf[64];
};

template <int D>
__global__ __launch_bounds__(1024) void k_vl_walk(const VlModel *__restrict__ models, const int *__restrict__ p0,
                                                  const int *__restrict__ srcs, const int *__restrict__ wgts,
                                                  const float *__restrict__ logA, const float *__restrict__ logE,
                                                  int b, int L, int q, unsigned short *__restrict__ bp,
                                                  int *__restrict__ path, double *__restrict__ score) {
    __shared__ VlWalkLds s;
    extern __shared__ int dyn[];                          // D = 0, q <= VL_DENSE_LDS: Q(log A) [i * q + j];
                                                          // afterwards the backtrace's staged rows
    const long long row = blockIdx.x;
    const int m = (int)(row / b), j = threadIdx.x, w = j >> 6, nw = blockDim.x >> 6;
    const VlModel &M = models[m];
    if (M.mode != D) return;                              // another instantiation serves this model
    const bool act = j < q;
    const float *Am = logA + (size_t)m * q * q;
    const bool alds = D == 0 && q <= VL_DENSE_LDS;
    if (alds) {
        for (int x = j; x < q * q; x += blockDim.x) dyn[x] = vquant(Am[x]);
    }
    int sv[D > 0 ? D : 1], wv[D > 0 ? D : 1];
    if constexpr (D > 0) {
        const int jj = act ? j : 0;
#pragma unroll
        for (int x = 0; x < D; ++x) {
            sv[x] = srcs[((size_t)m * q + jj) * VL_DMAX + x];
            wv[x] = wgts[((size_t)m * q + jj) * VL_DMAX + x];
        }
    }
    const int a_off = M.a_off;
    const float *Er = logE + (size_t)row * L * q;
    unsigned short *bpr = bp + (size_t)row * L * q;
    auto publish = [&](int buf, int d) {                  // this step's vector and its per-wave (max, lowest argmax)
        s.d[buf][j] = d;
        const int mx = mq_wave_max_i(d);
        const unsigned long long hit = __builtin_amdgcn_ballot_w64(d == mx);
        if ((j & 63) == 0) { s.wmx[buf][w] = mx; s.warg[buf][w] = 64 * w + __builtin_ctzll(hit); }
    };
    auto best_of = [&](int buf, int &istar) {             // maximum of a published vector, lowest index
        int mx = s.wmx[buf][0];
        istar = s.warg[buf][0];
        for (int x = 1; x < nw; ++x) {
            const int v = s.wmx[buf][x];
            if (v > mx) { mx = v; istar = s.warg[buf][x]; }
        }
        return mx;
    };
    publish(0, act ? p0[(size_t)m * q + j] + vquant(Er[j]) : VL_NEG);
    __syncthreads();
    long long base = 0;
    float en = (L > 1 && act) ? Er[(size_t)q + j] : 0.f;
    for (int t = 1; t < L; ++t) {
        const int cur = (t - 1) & 1;
        const float ef = en;
        if (t + 1 < L && act) en = Er[(size_t)(t + 1) * q + j];
        int istar;
        const int mx = best_of(cur, istar);
        int best, arg;
        if constexpr (D > 0) {
            int cand[D];
#pragma unroll
            for (int x = 0; x < D; ++x) cand[x] = s.d[cur][sv[x]] + wv[x];
            best = mx + a_off;
#pragma unroll
            for (int x = 0; x < D; ++x) best = max(best, cand[x]);
            arg = 0x7fffffff;
#pragma unroll
            for (int x = D - 1; x >= 0; --x) arg = cand[x] == best ? sv[x] : arg;
            arg = (mx + a_off == best) ? min(arg, istar) : arg;
        } else {
            best = VL_NEG - 0x20000000;
            arg = 0;
            if (alds) {
                for (int i = 0; i < q; ++i) {
                    const int c = s.d[cur][i] + dyn[i * q + (act ? j : 0)];
                    if (c > best) { best = c; arg = i; }
                }
            } else {
                for (int i = 0; i < q; ++i) {
                    const int c = s.d[cur][i] + vquant(Am[(size_t)i * q + (act ? j : 0)]);
                    if (c > best) { best = c; arg = i; }
                }
            }
        }
        base += mx;
        if (act) bpr[(size_t)t * q + j] = (unsigned short)arg;
        publish(t & 1, act ? best + vquant(ef) - mx : VL_NEG);
        __syncthreads();
    }
    int sfin;
    const int mxl = best_of((L - 1) & 1, sfin);
    if (j == 0) score[row] = (double)(base + mxl) / (double)VQ_SCALE;
    // backtrace: blocks of RB positions, their backpointer rows staged in LDS by all lanes, lane 0 walks them,
    // the block's path entries leave coalesced
    int *pr = path + (size_t)row * L;
    unsigned short *rows = reinterpret_cast<unsigned short *>(alds ? dyn : s.d[0]);
    int rb = (alds ? VL_DENSE_LDS * VL_DENSE_LDS * 4 : (int)sizeof(s.d)) / (q * 2);
    rb = rb < 64 ? rb : 64;
    int st = sfin;                                        // lane 0: state at position t1
    for (int t1 = L - 1; t1 >= 1; t1 -= rb) {
        const int t0 = t1 - rb + 1 > 1 ? t1 - rb + 1 : 1;
        __syncthreads();                                  // the previous block's rows / pbuf are consumed
        const size_t n = (size_t)(t1 - t0 + 1) * q;
        for (size_t x = j; x < n; x += blockDim.x) rows[x] = bpr[(size_t)t0 * q + x];
        __syncthreads();
        if (j == 0)
            for (int t = t1; t >= t0; --t) {
                s.pbuf[t - t0] = st;
                st = rows[(size_t)(t - t0) * q + st];
            }
        __syncthreads();
        if (j <= t1 - t0) pr[t0 + j] = s.pbuf[j];
    }
    if (j == 0) pr[0] = st;
}

// ------------------------------------------------------------------ per-position tiles
// Operand keys.  With p = d_{t-1}[i] - M_{t-1} <= 0 (the row's previous maximum subtracted while staging) and
// c = Q(logA[i][j]) - a_max in [-2^27, 0], a candidate is v = p + c <= 0, and the winner v* >= c[i*][j] >= -2^27.
// Keys, 32-bit signed:
//   P = (max(p, -2^28 + 1) + 2^27 - 1) * 16            in [-2^31, 2^31 - 16]
//   C = c * 16 + 15 - i % 16                            in [-2^31, 15]
//   key = sat(P + C)                                    (v_add_i32 with clamp)
// For the winner p >= v* >= -2^27 is not clamped and 16 (v* + 2^27 - 1) + 15 - i%16 lies in [-16, 2^31 - 1]: its
// key is exact.  Any other candidate either has an exact key, ordered by (v, lowest i%16) — ties in v resolve to
// the lower index within the slab of 16 — or a true value < -2^27 <= v*, and then a key below -16 (clamping p to
// -2^28 + 1 only lowers v, saturation only clamps at INT_MIN): it never wins.  A slab's maximum key is therefore
// (best value, lowest index attaining it) of the slab; across slabs, in increasing order, a slab replaces the
// running best only with a strictly greater VALUE: key > (running | 15).
__global__ __launch_bounds__(256) void k_vl_init(const int *__restrict__ p0, const float *__restrict__ logE,
                                                 int b, int L, int q, int ncolt, int *__restrict__ P,
                                                 int *__restrict__ pm, long long *__restrict__ base) {
    const long long row = blockIdx.x;
    const int m = (int)(row / b), tid = threadIdx.x;
    __shared__ int red[4];
    const float *Er = logE + (size_t)row * L * q;
    int *Pr = P + (size_t)row * q;
    int mx = VL_NEG;
    for (int j = tid; j < q; j += 256) {
        const int d = p0[(size_t)m * q + j] + vquant(Er[j]);
        Pr[j] = d;
        mx = max(mx, d);
    }
    mx = vl_wave_max(mx);
    if ((tid & 63) == 0) red[tid >> 6] = mx;
    __syncthreads();
    if (tid < ncolt) pm[(size_t)row * ncolt + tid] = max(max(red[0], red[1]), max(red[2], red[3]));
    if (tid == 0) base[row] = 0;
}

// grid (ncolt, k * ceil(b / BM)), 256 threads: thread (ty, tx) owns rows ty*4 .. +3, columns tx*4 .. +3 of the tile
__global__ __launch_bounds__(256) void k_vl_tile(const VlModel *__restrict__ models, const float *__restrict__ logA,
                                                 const float *__restrict__ logE, int b, int L, int q, int t, int ncolt,
                                                 const int *__restrict__ Pin, const int *__restrict__ pmin,
                                                 int *__restrict__ Pout, int *__restrict__ pmout,
                                                 long long *__restrict__ base, unsigned short *__restrict__ bp) {
    __shared__ __attribute__((aligned(16))) int As[VL_BK][VL_BM];
    __shared__ __attribute__((aligned(16))) int Bs[VL_BK][VL_BN];
    __shared__ int Ms[VL_BM];
    __shared__ int red[VL_BM][17];
    const int nrt = (b + VL_BM - 1) / VL_BM;
    const int m = blockIdx.y / nrt, r0 = (blockIdx.y % nrt) * VL_BM, c0 = blockIdx.x * VL_BN;
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const long long rowbase = (long long)m * b;          // global row of sequence 0 of this model
    const int a_max = models[m].a_max;
    const float *Am = logA + (size_t)m * q * q;
    // the previous maximum of each row (partials of the previous launch) -> frame of this step
    if (tid < VL_BM) {
        int mx = VL_NEG;
        if (r0 + tid < b) {
            const int *pr = pmin + (size_t)(rowbase + r0 + tid) * ncolt;
            for (int c = 0; c < ncolt; ++c) mx = max(mx, pr[c]);
            if (blockIdx.x == 0) base[rowbase + r0 + tid] += mx;
        }
        Ms[tid] = mx;
    }
    __syncthreads();
    int key[4][4], sl[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) { key[a][c] = VL_KEY_MIN; sl[a][c] = 0; }
    for (int k0 = 0; k0 < q; k0 += VL_BK) {
        // stage: As[kk][r] = P key of (row r, source k0 + kk), Bs[kk][c] = C key of (source k0 + kk, column c)
        for (int x = tid; x < VL_BK * VL_BM; x += 256) {
            const int r = x / VL_BK, kk = x % VL_BK, i = k0 + kk;
            int v = VL_KEY_MIN;
            if (r0 + r < b && i < q) {
                int p = Pin[(size_t)(rowbase + r0 + r) * q + i] - Ms[r];
                p = max(p, -(1 << 28) + 1);
                v = (p + (1 << 27) - 1) * 16;
            }
            As[kk][r] = v;
        }
        for (int x = tid; x < VL_BK * VL_BN; x += 256) {
            const int kk = x / VL_BN, c = x % VL_BN, i = k0 + kk, jcol = c0 + c;
            int v = VL_KEY_MIN;
            if (i < q && jcol < q) v = (vquant(Am[(size_t)i * q + jcol]) - a_max) * 16 + (15 - kk);
            Bs[kk][c] = v;
        }
        __syncthreads();
        int sm[4][4];
#pragma unroll
        for (int kk = 0; kk < VL_BK; ++kk) {
            const i4 pa = *reinterpret_cast<const i4 *>(&As[kk][ty * 4]);
            const i4 cb = *reinterpret_cast<const i4 *>(&Bs[kk][tx * 4]);
            const int pv[4] = {pa.x, pa.y, pa.z, pa.w}, cv[4] = {cb.x, cb.y, cb.z, cb.w};
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const int kv = __builtin_elementwise_add_sat(pv[a], cv[c]);
                    sm[a][c] = kk == 0 ? kv : max(sm[a][c], kv);
                }
        }
        const int slab = k0 / VL_BK;
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const bool up = sm[a][c] > (key[a][c] | 15);
                key[a][c] = up ? sm[a][c] : key[a][c];
                sl[a][c] = up ? slab : sl[a][c];
            }
        __syncthreads();
    }
    // epilogue: score relative to the new frame, backpointers, per-tile row maxima
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int r = ty * 4 + a;
        const bool rok = r0 + r < b;
        const long long grow = rowbase + r0 + r;
        int rmx = VL_NEG;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int jcol = c0 + tx * 4 + c;
            if (rok && jcol < q) {
                const int v = (key[a][c] >> 4) - ((1 << 27) - 1) + a_max;      // (key values are relative to a_max)
                const int arg = sl[a][c] * VL_BK + 15 - (key[a][c] & 15);
                const size_t o = ((size_t)grow * L + t) * q + jcol;
                const int d = v + vquant(logE[o]);
                Pout[(size_t)grow * q + jcol] = d;
                bp[o] = (unsigned short)arg;
                rmx = max(rmx, d);
            }
        }
        red[r][tx] = rmx;
    }
    __syncthreads();
    if (tid < VL_BM && r0 + tid < b) {
        int mx = red[tid][0];
        for (int x = 1; x < 16; ++x) mx = max(mx, red[tid][x]);
        pmout[(size_t)(rowbase + r0 + tid) * ncolt + blockIdx.x] = mx;
    }
}

// one wave per sequence: the last maximum (lowest index) and the score, then lane 0 follows the backpointers
__global__ __launch_bounds__(64) void k_vl_final(const int *__restrict__ P, const long long *__restrict__ base,
                                                 const unsigned short *__restrict__ bp, int L, int q,
                                                 int *__restrict__ path, double *__restrict__ score) {
    const long long row = blockIdx.x;
    const int j = threadIdx.x;
    const int *Pr = P + (size_t)row * q;
    int mx = VL_NEG - 1, arg = 0x7fffffff;
    for (int x = j; x < q; x += 64) {
        const int v = Pr[x];
        if (v > mx) { mx = v; arg = x; }                  // per lane: increasing index, strict '>'
    }
    const int wm = vl_wave_max(mx);
    const int wa = -vl_wave_max(-(mx == wm ? arg : 0x7fffffff));
    if (j != 0) return;
    score[row] = (double)(base[row] + wm) / (double)VQ_SCALE;
    const unsigned short *bpr = bp + (size_t)row * L * q;
    int *pr = path + (size_t)row * L;
    int st = wa;
    for (int t = L - 1; t >= 1; --t) {
        pr[t] = st;
        st = bpr[(size_t)t * q + st];
    }
    pr[0] = st;
}

static void vl_walk_launch(const VlModel *models, const int *p0, const int *src, const int *wgt, const float *logA,
                           const float *logE, int k, int b, int L, int q, unsigned short *bp, int *path, double *score,
                           hipStream_t st) {
    const dim3 grid((unsigned)((size_t)k * b)), blk((unsigned)((q + 63) / 64 * 64));
    const size_t dl = q <= VL_DENSE_LDS ? (size_t)VL_DENSE_LDS * VL_DENSE_LDS * sizeof(int) : 0;
    hipLaunchKernelGGL(k_vl_walk<4>, grid, blk, 0, st, models, p0, src, wgt, logA, logE, b, L, q, bp, path, score);
    hipLaunchKernelGGL(k_vl_walk<8>, grid, blk, 0, st, models, p0, src, wgt, logA, logE, b, L, q, bp, path, score);
    hipLaunchKernelGGL(k_vl_walk<0>, grid, blk, dl, st, models, p0, src, wgt, logA, logE, b, L, q, bp, path, score);
}

static void vl_tile_launch(const VlModel *models, const int *p0, const float *logA, const float *logE, int k, int b,
                           int L, int q, const VlLayout &v, char *ws, unsigned short *bp, int *path, double *score,
                           hipStream_t st) {
    const size_t nr = (size_t)k * b;
    int *P[2] = {(int *)(ws + v.o_P), (int *)(ws + v.o_P) + nr * q};
    int *pm[2] = {(int *)(ws + v.o_pm), (int *)(ws + v.o_pm) + nr * v.ncolt};
    long long *base = (long long *)(ws + v.o_base);
    hipLaunchKernelGGL(k_vl_init, dim3((unsigned)nr), dim3(256), 0, st, p0, logE, b, L, q, v.ncolt, P[0], pm[0], base);
    const dim3 grid((unsigned)v.ncolt, (unsigned)(k * ((b + VL_BM - 1) / VL_BM)));
    for (int t = 1; t < L; ++t)
        hipLaunchKernelGGL(k_vl_tile, grid, dim3(256), 0, st, models, logA, logE, b, L, q, t, v.ncolt,
                           (const int *)P[(t - 1) & 1], (const int *)pm[(t - 1) & 1], P[t & 1], pm[t & 1], base, bp);
    // the final maximum: fold the last partials into base like the next launch would, then take the argmax
    hipLaunchKernelGGL(k_vl_final, dim3((unsigned)nr), dim3(64), 0, st, (const int *)P[(L - 1) & 1],
                       (const long long *)base, (const unsigned short *)bp, L, q, path, score);
}

extern "C" int hmm_viterbi_large_max_states(void) { return VL_MAX; }

extern "C" size_t hmm_viterbi_large_workspace_bytes(int k, int b, int L, int q) {
    if (k < 1 || b < 1 || L < 1 || q < 1 || q > VL_MAX) return 0;
    VlLayout v;
    vl_layout(k, b, L, q, &v);
    return v.total;
}

extern "C" int hmm_viterbi_large(const float *logA, const float *logpi, const float *logE, int k, int b, int L, int q,
                                 int32_t *path, double *score, void *workspace, size_t workspace_bytes, void *stream) {
    if (k < 1 || b < 1 || L < 1 || q < 1) return HMM_ERR_BAD_SHAPE;
    if (q > VL_MAX) return HMM_ERR_Q_UNSUPPORTED;
    if (!logA || !logpi || !logE || !path || !score || !workspace) return HMM_ERR_NULL_POINTER;
    VlLayout v;
    vl_layout(k, b, L, q, &v);
    if (workspace_bytes < v.total || ((uintptr_t)workspace & 255)) return HMM_ERR_WORKSPACE;
    char *ws = (char *)workspace;
    hipStream_t st = (hipStream_t)stream;
    VlModel *models = (VlModel *)(ws + v.o_model);
    int *p0 = (int *)(ws + v.o_p0), *src = (int *)(ws + v.o_src), *wgt = (int *)(ws + v.o_wgt);
    unsigned short *bp = (unsigned short *)(ws + v.o_bp);
    const int route = opt(HMM_OPT_VLARGE);
    const bool walk = q <= VL_WALK_MAX && (route == 1 || (route != 2 && q <= VL_Q_WALK));
    hipLaunchKernelGGL(k_vl_prep, dim3((unsigned)k), dim3(1024), 0, st, logA, logpi, models, p0, src, wgt, q,
                       walk ? 1 : 0, opt(HMM_OPT_FORCE_DENSE) == 1 ? 1 : 0);
    if (walk)
        vl_walk_launch(models, p0, src, wgt, logA, logE, k, b, L, q, bp, path, score, st);
    else
        vl_tile_launch(models, p0, logA, logE, k, b, L, q, v, ws, bp, path, score, st);
    return check_launch();
}
