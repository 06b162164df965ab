// hmm_viterbi_scan.inc — time-parallel Viterbi for up to 64 states (hmm_viterbi_scan), included after
// hmm_viterbi.inc whose Q16 definition, k_mq_prep / MqModel, MqCand and mq_backtrace it shares.
//
// Semantics (oracle/viterbi.py, unchanged): Q(x) = rint(clip(x, -1024, 1024) * 65536),
//     d_t[j] = max_i (d_{t-1}[i] + Q(logA[i][j])) + Q(logE_t[j]),  lowest index wins every tie,
// score = d_{L-1} / 2^16.  The plan is the three-phase plan of hmm_viterbi.inc with q x q max-plus chunk
// operators in tiles of QT = 32 (q <= 32) or 64 states:
//   k_vs_prep       Q(logA) (both orientations) and Q(logpi) per model; k_mq_prep classifies the model.
//   k_vs_reduce     one wave per chunk, lane = START state: every lane runs the same vector recursion from
//                   its own unit start, so predecessor lists and weights are wave-uniform (scalar loads) and
//                   nothing crosses lanes.  Sparse models (k_mq_prep: no state with more than 8 explicit
//                   predecessors) visit their predecessors plus the one off-edge candidate "best previous
//                   score + matrix minimum" (exact, k_vit_prep's rule); others visit all q candidates.
//   k_vs_scan       scores entering every chunk, final state and score — one level, or two
//                   (k_vs_compose: the operator of every group of ~sqrt(C) chunks; k_vs_scan over the groups;
//                   k_vs_scan over the chunks of every group in parallel).
//   k_vs_apply      one wave per chunk, lane = state: the step of k_mq_viterbi from the TRUE entering scores,
//                   one backpointer byte per (position, state), and the map "state at chunk end -> state
//                   before the chunk".
//   k_vs_scan_bwd / k_vs_bwd_compose / k_vs_bwd_inner   state at every chunk end, one or two levels.
//   k_vs_backtrace  every chunk in parallel (mq_backtrace on the chunk's backpointer rows).
//
// Exactness.  Integer max-plus is exactly associative, so operators, entering scores and the final score are
// the integers of the serial recursion.  Ties: backpointers are formed ONLY in k_vs_apply, from exact entering
// scores with k_mq_viterbi's own step (explicit predecessors in increasing index with strict '>', the off-edge
// candidate wins a tie only with a lower index); the operators contribute values only.
// Nothing saturates, whatever q: every term Q(.) lies in [-2^26, 2^26] and after clamping every edge exists, so
//   (a) one COLUMN of an operator (the scores after >= 1 steps from one start state) has a spread <= 2^28: the
//       first step gives A[i][j] + E[j] in [-2^27, 2^27]; later any state is reached from the step's best
//       predecessor at >= -2^27 while the best score grows by <= 2^27;
//   (b) the best scores of two columns differ by <= 2^28: from start i take the first edge of the other
//       column's best path (>= -2^26 against <= 2^26, the emission is shared) and follow that path.
// An operator is therefore stored PER COLUMN: 32-bit entries relative to the column's maximum (in [-2^28, 0]),
// a 32-bit column base relative to the operator's largest base (in [-2^28, 0]) and ONE 64-bit base per operator.
// A composition or hop adds three such terms: >= -3 * 2^28 > -2^31.  Padded rows / columns hold VS_NEG = -2^30:
// below every real candidate sum, and VS_NEG plus any two real terms, or VS_NEG + VS_NEG, is still >= -2^31.
// Inside a chunk the reduce keeps each lane's vector relative to the maximum of the step before last
// (entries in [-2^27, 2^27] + one step's growth), with a 64-bit base per lane; the apply pass keeps
// k_mq_viterbi's frame ([-2^29, 2^27]).  The same bounds hold for composed (group) operators: they are the
// operators of longer chunks.
//
// Every offset into logE, path and the backpointers is 64-bit; everything runs in order on `stream`.
//
// VsPlan::seq_start (hmm_viterbi_scan: always 1) says whether the tensor begins at position 0 of its sequences.  A time
// slab that does not (hmm_seqshard_vscan.inc) has no first observation: its chunk 0 is an ordinary chunk with an
// operator column per start state, entering scores, a backpointer row at its step 0 and a valid end -> before map.
// "First chunk of a sequence" is `c == 0 && seq_start` throughout.

#define VS_NEG (-0x40000000)
#define VS_ET 16          // steps per staged emission tile

struct VsModel {              // per model, in the workspace
    int aq[64 * 64];          // Q(logA[i][j]) at [i * 64 + j]; VS_NEG outside q x q
    int aqT[64 * 64];         // the same at [j * 64 + i]: the candidates of destination j are contiguous
    int p0[64];               // Q(logpi)
};

struct VsPlan {
    int k, b, L, q, QT, NB, T, C, G, gsize;
    int seq_start;            // 1: position 0 of the tensor is position 0 of the sequences
    long long nchains;
    size_t o_mq, o_model, o_vops, o_vrb, o_vmb, o_dstart, o_forig, o_send, o_sfinal;
    size_t o_gvops, o_gvrb, o_gvmb, o_gdstart, o_gforig, o_gsend, o_bp, total;
};

// One chunk per wave, so a chunk is a serial walk of T steps for its wave and every chunk costs a QT x QT
// operator in the scans: aim at ~8192 chunks (8 waves per SIMD), never below the T^3 = 2.25 L of choose_T
// (in-chunk steps against scan hops), never above MAX_T.
static int vs_choose_T(long long NB, int L) {
    const int f = opt(HMM_OPT_CHUNK);
    if (f >= 16 && f <= MAX_T && f % 16 == 0) return f;
    long long t = NB * (long long)L / 8192;
    long long tb = 16;
    while (tb * tb * tb * 4 < 9ll * L && tb < MAX_T) tb += 16;
    if (t < tb) t = tb;
    t = (t + 15) / 16 * 16;
    if (t > MAX_T) t = MAX_T;
    const long long lmax = ((long long)L + 15) / 16 * 16;
    if (t > lmax) t = lmax;
    return (int)t;
}

static int make_vsplan(int k, int b, int L, int q, VsPlan *v) {
    if (k < 1 || b < 1 || L < 1 || q < 1) return HMM_ERR_BAD_SHAPE;
    if ((long long)k * b > (1ll << 24)) return HMM_ERR_BAD_SHAPE;
    if (q > MQ_MAX) return HMM_ERR_Q_UNSUPPORTED;
    v->k = k; v->b = b; v->L = L; v->q = q;
    v->seq_start = 1;
    v->QT = q <= 32 ? 32 : 64;
    v->NB = k * b;
    v->T = vs_choose_T(v->NB, L);
    v->C = (L + v->T - 1) / v->T;
    v->nchains = (long long)v->NB * v->C;
    if (v->nchains > 0x7fffffffll) return HMM_ERR_BAD_SHAPE;
    v->G = 0; v->gsize = 0;
    if (v->C >= SCAN2_MIN_C) {
        int gs = 1;
        while (gs * gs < v->C) ++gs;
        v->gsize = gs;
        v->G = (v->C + gs - 1) / gs;
    }
    const size_t QT = (size_t)v->QT, nc = (size_t)v->nchains, ng = (size_t)v->NB * (v->G > 0 ? v->G : 1);
    size_t off = 0;
    v->o_mq = off;      off = align_up(off + (size_t)k * sizeof(MqModel));
    v->o_model = off;   off = align_up(off + (size_t)k * sizeof(VsModel));
    v->o_vops = off;    off = align_up(off + nc * QT * QT * sizeof(int));
    v->o_vrb = off;     off = align_up(off + nc * QT * sizeof(int));
    v->o_vmb = off;     off = align_up(off + nc * sizeof(long long));
    v->o_dstart = off;  off = align_up(off + nc * QT * sizeof(int));
    v->o_forig = off;   off = align_up(off + nc * 64);
    v->o_send = off;    off = align_up(off + nc * sizeof(int));
    v->o_sfinal = off;  off = align_up(off + (size_t)v->NB * sizeof(int));
    v->o_gvops = off;   off = align_up(off + ng * QT * QT * sizeof(int));
    v->o_gvrb = off;    off = align_up(off + ng * QT * sizeof(int));
    v->o_gvmb = off;    off = align_up(off + ng * sizeof(long long));
    v->o_gdstart = off; off = align_up(off + ng * QT * sizeof(int));
    v->o_gforig = off;  off = align_up(off + ng * 64);
    v->o_gsend = off;   off = align_up(off + ng * sizeof(int));
    v->o_bp = off;      off = align_up(off + (size_t)v->NB * (size_t)L * 64);      // 64-byte rows, as k_mq_viterbi's
    v->total = off;
    return HMM_OK;
}

__global__ __launch_bounds__(64) void k_vs_prep(const float *__restrict__ logA, const float *__restrict__ logpi,
                                                VsModel *__restrict__ models, int q) {
    const int m = blockIdx.x, j = threadIdx.x;
    VsModel &M = models[m];
    const float *Am = logA + (size_t)m * q * q;
    for (int i = 0; i < 64; ++i) {
        const int v = (i < q && j < q) ? vquant(Am[(size_t)i * q + j]) : VS_NEG;
        M.aq[i * 64 + j] = v;
        M.aqT[j * 64 + i] = v;
    }
    M.p0[j] = j < q ? vquant(logpi[(size_t)m * q + j]) : VS_NEG;
}

__device__ __forceinline__ long long vs_wave_max_ll(long long v) {
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) { const long long o = __shfl_xor(v, s, 64); v = o > v ? o : v; }
    return v;
}

// Emission rows of one chunk, VS_ET steps at a time: lane = state loads its own column of the next tile
// through branch-free raw buffer loads (rows past the sequence are outside the descriptor and read 0) while
// the current tile is walked; quantised once while staging.
struct VsEmis {
    const float *Er;          // row t0 of the sequence
    int rows, rowb, voff;     // rows left in the SEQUENCE from t0 on
    bool act;
};
__device__ __forceinline__ void vs_fetch(const VsEmis &s, int tile, float (&r)[VS_ET]) {
    const long long r0 = (long long)tile * VS_ET;
    const long long rem = ((long long)s.rows - r0) * s.rowb;
    const __amdgpu_buffer_rsrc_t rs =
        make_rsrc(s.Er + r0 * (s.rowb / 4), rem > 0 ? (unsigned long long)(rem < (1ll << 20) ? rem : (1ll << 20)) : 0ull);
#pragma unroll
    for (int u = 0; u < VS_ET; ++u)
        r[u] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, s.voff + u * s.rowb, 0, 0));
}
__device__ __forceinline__ void vs_stage(const VsEmis &s, const float (&r)[VS_ET], int (*es)[64], int lane) {
#pragma unroll
    for (int u = 0; u < VS_ET; ++u) es[u][lane] = s.act ? vquant(r[u]) : 0;
}

// ------------------------------------------------------------------ reduce: the operator of every chunk
// xs[buffer][state][lane]: lane's score vector, relative to the lane's frame: true = x + base - mprev, where
// mprev is the vector's maximum as stored (the frame moves by the previous maximum every step, so that the
// off-edge candidate is simply a_off in the new frame).  D = 0: all q candidates; else D explicit predecessors
// (padded by k_mq_prep with weight MQ_NEG, never the maximum) plus the off-edge candidate.
template <int QT, int D>
__device__ __forceinline__ void vs_reduce_chunk(const VsEmis &em, const MqModel &S, const VsModel &M, int (*xs)[QT][64],
                                                int (*es)[64], int q, int len, bool first, int lane,
                                                int &mprev_out, long long &base_out, int &cur_out) {
    const int il = lane < q ? lane : 0;                  // idle lanes repeat start state 0 (never stored)
    const int a_off = S.a_off;
    float r[VS_ET];
    vs_fetch(em, 0, r);
    int cur = 0, mprev = 0;
    long long base = 0;
    for (int tile = 0; tile * VS_ET < len; ++tile) {
        vs_stage(em, r, es, lane);
        vs_fetch(em, tile + 1, r);
        const int nst = min(VS_ET, len - tile * VS_ET);
        for (int u = 0; u < nst; ++u) {
            const int *xc = &xs[cur][0][0];
            int *xn = &xs[cur ^ 1][0][0];
            int mx = -0x7fffffff;
            if (tile == 0 && u == 0) {
                // a max-plus unit vector has no bounded spread: start AFTER the first step, A[i][.] + E (pi + E in
                // the first chunk of a sequence, the same in every column)
                for (int j = 0; j < q; ++j) {
                    const int y = (first ? M.p0[j] : M.aq[il * 64 + j]) + es[0][j];
                    xn[j * 64 + lane] = y;
                    mx = max(mx, y);
                }
            } else if constexpr (D == 0) {
                for (int j = 0; j < q; ++j) {
                    const int *a = &M.aqT[j * 64];
                    int best = xc[lane] + a[0];
                    for (int i = 1; i < q; ++i) best = max(best, xc[i * 64 + lane] + a[i]);
                    const int y = best - mprev + es[u][j];
                    xn[j * 64 + lane] = y;
                    mx = max(mx, y);
                }
            } else {
                const int rest = mprev + a_off;
                for (int j = 0; j < q; ++j) {
                    int best = rest;
#pragma unroll
                    for (int x = 0; x < D; ++x) best = max(best, xc[S.src[j][x] * 64 + lane] + S.wgt[j][x]);
                    const int y = best - mprev + es[u][j];
                    xn[j * 64 + lane] = y;
                    mx = max(mx, y);
                }
            }
            base += mx;
            mprev = mx;
            cur ^= 1;
        }
    }
    mprev_out = mprev; base_out = base; cur_out = cur;
}

template <int QT>
__global__ __launch_bounds__(64) void k_vs_reduce(const float *__restrict__ logE, const MqModel *__restrict__ mq,
                                                  const VsModel *__restrict__ models, int *__restrict__ vops,
                                                  int *__restrict__ vrb, long long *__restrict__ vmb, VsPlan p) {
    __shared__ int xs[2][QT][64];
    __shared__ int es[VS_ET][64];
    const int lane = threadIdx.x, q = p.q;
    const long long chain = blockIdx.x;
    const int row = (int)(chain / p.C), c = (int)(chain - (long long)row * p.C), m = row / p.b;
    const int t0 = c * p.T, len = min(p.T, p.L - t0);
    const MqModel &S = mq[m];
    const VsModel &M = models[m];
    VsEmis em;
    em.Er = logE + ((size_t)row * p.L + t0) * q;
    em.rows = p.L - t0; em.rowb = q * (int)sizeof(float);
    em.act = lane < q; em.voff = em.act ? lane * 4 : 0;
    const int mode = __builtin_amdgcn_readfirstlane(S.mode);
    const bool first = c == 0 && p.seq_start;
    int mprev, cur;
    long long base;
    if (mode == 0) vs_reduce_chunk<QT, 0>(em, S, M, xs, es, q, len, first, lane, mprev, base, cur);
    else if (mode == 3) vs_reduce_chunk<QT, 3>(em, S, M, xs, es, q, len, first, lane, mprev, base, cur);
    else if (mode == 4) vs_reduce_chunk<QT, 4>(em, S, M, xs, es, q, len, first, lane, mprev, base, cur);
    else vs_reduce_chunk<QT, 8>(em, S, M, xs, es, q, len, first, lane, mprev, base, cur);
    // column `lane`: entries relative to its maximum, base relative to the operator's largest
    const bool act = lane < q;
    const long long mb = vs_wave_max_ll(act ? base : (long long)0x8000000000000000ll);
    if (lane < QT) {
        int *V = vops + (size_t)chain * QT * QT + lane;
        for (int j = 0; j < QT; ++j) V[j * QT] = (act && j < q) ? xs[cur][j][lane] - mprev : VS_NEG;
        vrb[(size_t)chain * QT + lane] = act ? (int)(base - mb) : 0;
    }
    if (lane == 0) vmb[chain] = mb;
}

// ------------------------------------------------------------------ forward scan over operators
// Lane j = end state holds row j of the next operator (fetched one hop ahead).  A hop: u[i] = rel[i] + rb[i],
// rel'[j] = max_i (u[i] + V[j][i]) re-normalised to maximum 0, base += mb + maximum.
// G == 0: one block per sequence over its C operators (chunks, or the groups of the two-level scan): records the
// scores entering operator 1 .. C-1, the final state and the score.  G > 0: one block per (sequence, group):
// from the scores entering the group (gdstart; group 0 starts the sequence) records those entering each of its chunks.
// seq_start == 0 (a time slab behind the first one): operator 0 is an ordinary operator — the top level starts from
// the scores entering the slab (gdstart, one row per sequence), records those entering operator 0 as well and, with
// sfinal == NULL, leaves the sequence's final state and score alone (they are not this slab's to know).
// SLABS (hmm_seqshard_vscan.inc): the top level over the gathered operators of R time slabs, whose column bases
// arrive as one int64 per column (mb: [sequence][slab][QT], rb unused): the hop forms the operator's largest base and
// the 32-bit relative column bases itself.  The scores entering slab r also go to entry[sequence][QT].
template <int QT, bool SLABS>
__global__ __launch_bounds__(64) void k_vs_scan(const int *__restrict__ ops, const int *__restrict__ rb,
                                                const long long *__restrict__ mb, int *__restrict__ dstart,
                                                const int *__restrict__ gdstart, int *__restrict__ sfinal,
                                                double *__restrict__ score, int q, int C, int G, int gsize,
                                                int seq_start, int *__restrict__ entry, int r) {
    const int lane = threadIdx.x, jl = lane & (QT - 1);
    const bool act = lane < q;
    const bool top = G == 0;
    int seq = blockIdx.x, grp = 0, c_begin = 0, c_end = C;
    if (!top) {
        seq = blockIdx.x / G;
        grp = blockIdx.x - seq * G;
        c_begin = grp * gsize;
        c_end = min(C, c_begin + gsize);
    }
    const size_t ch0 = (size_t)seq * C;
    int rel;
    long long base = 0;
    if (grp == 0 && seq_start) {                             // the first chunk's columns all hold the score vector
        if constexpr (SLABS) {
            rel = act ? ops[(ch0 * QT + jl) * QT] : 0;
            base = mb[ch0 * QT];
        } else {
            rel = act ? ops[(ch0 * QT + jl) * QT] + rb[ch0 * QT] : 0;
            base = mb[ch0];
        }
        c_begin = 1;
    } else {
        rel = act ? gdstart[(top ? (size_t)seq : (size_t)seq * G + grp) * QT + jl] : 0;
    }
    i4 nv[QT / 4];
    int nrb = 0;
    long long nmb = 0;
    auto fetch = [&](int c) {
        const i4 *R = reinterpret_cast<const i4 *>(ops + ((ch0 + c) * QT + jl) * QT);
#pragma unroll
        for (int u = 0; u < QT / 4; ++u) nv[u] = R[u];
        if constexpr (SLABS) {
            const long long cb = act ? mb[(ch0 + c) * QT + jl] : (long long)0x8000000000000000ll;
            nmb = vs_wave_max_ll(cb);
            nrb = act ? (int)(cb - nmb) : 0;
        } else {
            nrb = rb[(ch0 + c) * QT + jl];
            nmb = mb[ch0 + c];
        }
    };
    if (c_begin < c_end) fetch(c_begin);
    for (int c = c_begin; c < c_end; ++c) {
        if (lane < QT) dstart[(ch0 + c) * QT + lane] = rel;
        if constexpr (SLABS) {
            if (c == r && lane < QT) entry[(size_t)seq * QT + lane] = rel;
        }
        if (!top && c + 1 == c_end) break;                   // the group's last operator leads out of it
        i4 v[QT / 4];
#pragma unroll
        for (int u = 0; u < QT / 4; ++u) v[u] = nv[u];
        const int u0 = rel + nrb;                            // idle lanes: 0 against VS_NEG entries
        const long long cmb = nmb;
        if (c + 1 < c_end) fetch(c + 1);
        int best = VS_NEG * 2 + 1;
#pragma unroll
        for (int u = 0; u < QT / 4; ++u) {
            best = max(best, __builtin_amdgcn_readlane(u0, 4 * u) + v[u].x);
            best = max(best, __builtin_amdgcn_readlane(u0, 4 * u + 1) + v[u].y);
            best = max(best, __builtin_amdgcn_readlane(u0, 4 * u + 2) + v[u].z);
            best = max(best, __builtin_amdgcn_readlane(u0, 4 * u + 3) + v[u].w);
        }
        const int mx = mq_wave_max_i(act ? best : VS_NEG * 2 + 1);
        rel = act ? best - mx : 0;
        base += cmb + mx;
    }
    if (top && sfinal) {
        const unsigned long long ball = __builtin_amdgcn_ballot_w64(act && rel == 0);
        if (lane == 0) {
            sfinal[seq] = __builtin_ctzll(ball);             // lowest index among the best
            score[seq] = (double)base / (double)VQ_SCALE;
        }
    }
}

// One wave per (sequence, group): W <- V_c (x) W over the group's chunks.  Lane k = start state of the group owns
// column k of W (through LDS between hops, in registers within one); rows of V_c are wave-uniform.
// COLS64 (hmm_seqshard_vscan.inc, a slab's operator for the exchange): one int64 base per column to gvmb[wave][QT]
// (0 in the lanes from q on) instead of the 32-bit relative bases and the operator's largest; gvrb is not written.
template <int QT, bool COLS64>
__global__ __launch_bounds__(64) void k_vs_compose(const int *__restrict__ vops, const int *__restrict__ vrb,
                                                   const long long *__restrict__ vmb, int *__restrict__ gvops,
                                                   int *__restrict__ gvrb, long long *__restrict__ gvmb, int q, int C,
                                                   int G, int gsize) {
    __shared__ int wl[QT][64];
    const int lane = threadIdx.x, kl = lane & (QT - 1);
    const bool act = lane < q;
    const size_t wv = blockIdx.x;
    const int seq = (int)(wv / G), grp = (int)(wv - (size_t)seq * G);
    const int c0 = grp * gsize, c1 = min(C, c0 + gsize);
    const size_t ch0 = (size_t)seq * C + c0;
    for (int m = 0; m < QT; ++m) wl[m][lane] = act ? vops[(ch0 * QT + m) * QT + kl] : 0;     // idle lanes: bounded filler
    long long cb = (long long)vrb[ch0 * QT + kl] + vmb[ch0];
    for (int c = c0 + 1; c < c1; ++c) {
        const size_t ch = (size_t)seq * C + c;
        int w[QT];
#pragma unroll
        for (int m = 0; m < QT; ++m) w[m] = wl[m][lane] + vrb[ch * QT + m];
        int mx = -0x7fffffff;
        for (int j = 0; j < q; ++j) {
            const int *Vr = vops + (ch * QT + j) * QT;
            int t = w[0] + Vr[0];
#pragma unroll
            for (int m = 1; m < QT; ++m) t = max(t, w[m] + Vr[m]);
            wl[j][lane] = t;
            mx = max(mx, t);
        }
        for (int j = 0; j < q; ++j) wl[j][lane] -= mx;
        cb += vmb[ch] + (long long)mx;
    }
    const long long mbv = vs_wave_max_ll(act ? cb : (long long)0x8000000000000000ll);
    if (lane < QT) {
        int *W = gvops + wv * QT * QT + lane;
        for (int m = 0; m < QT; ++m) W[m * QT] = (act && m < q) ? wl[m][lane] : VS_NEG;
        if constexpr (COLS64) gvmb[wv * QT + lane] = act ? cb : 0;
        else gvrb[wv * QT + lane] = act ? (int)(cb - mbv) : 0;
    }
    if (!COLS64 && lane == 0) gvmb[wv] = mbv;
}

// ------------------------------------------------------------------ apply: true scores, backpointers
// The step of k_mq_viterbi (D = 0: all candidates, column j of Q(logA) in QB registers; D = 4 serves the models
// k_mq_prep put in mode 3 or 4, D = 8 mode 8) from the scores entering the chunk.  og: the state before the
// chunk of the best path into state j — it starts as the lane's own index, so the first step leaves its argmax.
template <int QB, int D>
__global__ __launch_bounds__(64) void k_vs_apply(const float *__restrict__ logE, const MqModel *__restrict__ mq,
                                                 const VsModel *__restrict__ models, const int *__restrict__ dstart,
                                                 unsigned char *__restrict__ forig, unsigned char *__restrict__ bp,
                                                 VsPlan p) {
    __shared__ int es[VS_ET][64];
    const int j = threadIdx.x, q = p.q;
    const long long chain = blockIdx.x;
    const int row = (int)(chain / p.C), c = (int)(chain - (long long)row * p.C), m = row / p.b;
    const MqModel &S = mq[m];
    const int mode = __builtin_amdgcn_readfirstlane(S.mode);
    if (D == 0 ? mode != 0 : (D == 4 ? (mode != 3 && mode != 4) : mode != 8)) return;     // another instantiation has this model
    const VsModel &M = models[m];
    const int t0 = c * p.T, len = min(p.T, p.L - t0);
    const bool act = j < q;
    constexpr int NA = D ? 1 : QB;
    int acol[NA];
    i4 sa = {0, 0, 0, 0}, sb = sa, wa = sa, wb = sa;       // vector VALUES, not arrays (see k_mq_viterbi)
    if constexpr (D == 0) {
#pragma unroll
        for (int i = 0; i < QB; ++i) acol[i] = (act && i < q) ? M.aq[i * 64 + j] : 0;
    } else {
        sa = *reinterpret_cast<const i4 *>(&S.src[j][0]); wa = *reinterpret_cast<const i4 *>(&S.wgt[j][0]);
        if constexpr (D == 8) { sb = *reinterpret_cast<const i4 *>(&S.src[j][4]); wb = *reinterpret_cast<const i4 *>(&S.wgt[j][4]); }
    }
    auto pick = [](const i4 &a, const i4 &b, int x) {       // x is a constant after unrolling
        const i4 v = x < 4 ? a : b;
        return (x & 3) == 0 ? v.x : ((x & 3) == 1 ? v.y : ((x & 3) == 2 ? v.z : v.w));
    };
    const int a_off = S.a_off;
    constexpr int NR = QB / 16;
    VsEmis em;
    em.Er = logE + ((size_t)row * p.L + t0) * q;
    em.rows = p.L - t0; em.rowb = q * (int)sizeof(float);
    em.act = act; em.voff = act ? j * 4 : 0;
    unsigned char *bpr = bp + ((size_t)row * p.L + t0) * 64;
    const bool first = c == 0 && p.seq_start;
    int d = act ? (first ? 0 : dstart[(size_t)chain * p.QT + j]) : MQ_NEG;
    int og = j;
    float r[VS_ET];
    vs_fetch(em, 0, r);
    for (int tile = 0; tile * VS_ET < len; ++tile) {
        __builtin_amdgcn_wave_barrier();
        vs_stage(em, r, es, j);
        vs_fetch(em, tile + 1, r);
        __builtin_amdgcn_wave_barrier();
        const int nst = min(VS_ET, len - tile * VS_ET);
        for (int u = 0; u < nst; ++u) {
            const int e = es[u][j];
            int arg;
            if (first && tile == 0 && u == 0) {             // the sequence's first position: no transition into it
                d = act ? M.p0[j] + e : MQ_NEG;
                arg = j;
            } else if constexpr (D == 0) {
                int cand[QB];
                MqCand<QB, 0>::fill(d, j, acol, cand);      // lanes >= q hold MQ_NEG: never win
                int best = cand[0];
#pragma unroll
                for (int i = 1; i + 1 < QB; i += 2) best = max(max(best, cand[i]), cand[i + 1]);
                best = max(best, cand[QB - 1]);
                arg = QB - 1;
#pragma unroll
                for (int i = QB - 2; i >= 0; --i) arg = cand[i] == best ? i : arg;
                const int y = act ? best + e : MQ_NEG;
                const int mx = mq_wave_max_i(y);
                d = act ? y - mx : MQ_NEG;
            } else {
                int cand[D];
#pragma unroll
                for (int x = 0; x < D; ++x) cand[x] = __builtin_amdgcn_ds_bpermute(pick(sa, sb, x) * 4, d);
                const int mx = mq_wave_max_s<NR>(d);
                const int istar = __builtin_ctzll(__builtin_amdgcn_ballot_w64(d == mx));
                const int off = mx + a_off;
#pragma unroll
                for (int x = 0; x < D; ++x) cand[x] += pick(wa, wb, x);
                int best = off;
#pragma unroll
                for (int x = 0; x < D; ++x) best = max(best, cand[x]);
                d = act ? best + (e - mx) : MQ_NEG;
                arg = 64;
#pragma unroll
                for (int x = D - 1; x >= 0; --x) arg = cand[x] == best ? pick(sa, sb, x) : arg;
                arg = off == best ? min(arg, istar) : arg;
            }
            arg = act ? arg : 0;
            bpr[(size_t)(tile * VS_ET + u) * 64 + j] = (unsigned char)arg;
            og = __builtin_amdgcn_ds_bpermute(arg * 4, og);
        }
    }
    forig[(size_t)chain * 64 + j] = (unsigned char)(act ? og : 0);
}

// ------------------------------------------------------------------ backward scan: state at every chunk end
__global__ void k_vs_scan_bwd(const unsigned char *__restrict__ forig, const int *__restrict__ sfinal,
                              int *__restrict__ send, int NB, int C) {
    const int seq = blockIdx.x * blockDim.x + threadIdx.x;
    if (seq >= NB) return;
    const size_t chain0 = (size_t)seq * C;
    int s = sfinal[seq];
    for (int c = C - 1; c >= 0; --c) {
        send[chain0 + c] = s;
        if (c > 0) s = forig[(chain0 + c) * 64 + s];
    }
}

// two levels: the maps "state at chunk end -> state before the chunk" compose exactly
__global__ void k_vs_bwd_compose(const unsigned char *__restrict__ forig, unsigned char *__restrict__ gforig, int NB,
                                 int C, int G, int gsize) {
    const long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x;       // (sequence, group, end state)
    if (id >= (long long)NB * G * 64) return;
    const int j = (int)(id & 63);
    const long long wv = id >> 6;
    const int seq = (int)(wv / G), grp = (int)(wv - (long long)seq * G);
    const int c0 = grp * gsize, c1 = min(C, c0 + gsize);
    int s = j;
    for (int c = c1 - 1; c >= c0; --c) s = forig[((size_t)seq * C + c) * 64 + s] & 63;    // (chunk 0's map: read for a later time slab only)
    gforig[(size_t)wv * 64 + j] = (unsigned char)s;
}

__global__ void k_vs_bwd_inner(const unsigned char *__restrict__ forig, const int *__restrict__ gsend,
                               int *__restrict__ send, int NB, int C, int G, int gsize) {
    const long long wv = (long long)blockIdx.x * blockDim.x + threadIdx.x;       // (sequence, group)
    if (wv >= (long long)NB * G) return;
    const int seq = (int)(wv / G), grp = (int)(wv - (long long)seq * G);
    const int c0 = grp * gsize, c1 = min(C, c0 + gsize);
    const size_t chain0 = (size_t)seq * C;
    int s = gsend[wv];                              // state at the end of the group's last chunk
    for (int c = c1 - 1; c >= c0; --c) {
        send[chain0 + c] = s;
        if (c > c0) s = forig[(chain0 + c) * 64 + s];
    }
}

// ------------------------------------------------------------------ backtrace inside every chunk
// Position t0 - 1 belongs to the previous chunk (its end state came out of the backward scan), so the chunk's
// first backpointer row is not followed: exactly mq_backtrace's treatment of a sequence's first row.
__global__ __launch_bounds__(64) void k_vs_backtrace(const unsigned char *__restrict__ bp, const int *__restrict__ send,
                                                     int *__restrict__ path, VsPlan p) {
    __shared__ __attribute__((aligned(16))) MqBtLds btl;
    const long long chain = blockIdx.x;
    const int row = (int)(chain / p.C), c = (int)(chain - (long long)row * p.C);
    const int t0 = c * p.T, len = min(p.T, p.L - t0);
    const size_t pos = (size_t)row * p.L + t0;
    const int s = __builtin_amdgcn_readfirstlane(send[chain]);
    mq_backtrace(bp + pos * 64, path + pos, len, threadIdx.x, s, btl);
}

// ------------------------------------------------------------------ host entry
template <int QT>
static void vs_launch_apply(const float *logE, const VsPlan &v, char *ws, hipStream_t st) {
    const MqModel *cmq = (const MqModel *)(ws + v.o_mq);
    const VsModel *cm = (const VsModel *)(ws + v.o_model);
    const int *cd = (const int *)(ws + v.o_dstart);
    unsigned char *forig = (unsigned char *)(ws + v.o_forig), *bp = (unsigned char *)(ws + v.o_bp);
    const dim3 chains((unsigned)v.nchains), wave(64);
    hipLaunchKernelGGL((k_vs_apply<QT, 4>), chains, wave, 0, st, logE, cmq, cm, cd, forig, bp, v);
    hipLaunchKernelGGL((k_vs_apply<QT, 8>), chains, wave, 0, st, logE, cmq, cm, cd, forig, bp, v);
    hipLaunchKernelGGL((k_vs_apply<QT, 0>), chains, wave, 0, st, logE, cmq, cm, cd, forig, bp, v);
}

// the groups' maps (two levels): every chunk of a group composed, its first one included
static void vs_launch_group_maps(const VsPlan &v, char *ws, hipStream_t st) {
    const long long ngrp = (long long)v.NB * v.G;
    hipLaunchKernelGGL(k_vs_bwd_compose, dim3((unsigned)((ngrp * 64 + 255) / 256)), dim3(256), 0, st,
                       (const unsigned char *)(ws + v.o_forig), (unsigned char *)(ws + v.o_gforig), v.NB, v.C, v.G, v.gsize);
}

// from the state at the tensor's last position (sfinal): the state at every chunk end, then every chunk's backtrace
static void vs_launch_backward(const VsPlan &v, char *ws, int32_t *path, bool two, hipStream_t st) {
    const unsigned char *forig = (const unsigned char *)(ws + v.o_forig);
    const int *sfinal = (const int *)(ws + v.o_sfinal);
    int *send = (int *)(ws + v.o_send);
    const int NB = v.NB, C = v.C, G = v.G;
    const dim3 wave(64);
    if (!two) {
        hipLaunchKernelGGL(k_vs_scan_bwd, dim3((NB + 63) / 64), wave, 0, st, forig, sfinal, send, NB, C);
    } else {
        const unsigned ngrp = (unsigned)((long long)NB * G);
        int *gsend = (int *)(ws + v.o_gsend);
        hipLaunchKernelGGL(k_vs_scan_bwd, dim3((NB + 63) / 64), wave, 0, st, (const unsigned char *)(ws + v.o_gforig),
                           sfinal, gsend, NB, G);
        hipLaunchKernelGGL(k_vs_bwd_inner, dim3((ngrp + 63) / 64), wave, 0, st, forig, (const int *)gsend, send, NB, C, G,
                           v.gsize);
    }
    hipLaunchKernelGGL(k_vs_backtrace, dim3((unsigned)v.nchains), wave, 0, st, (const unsigned char *)(ws + v.o_bp),
                       (const int *)send, path, v);
}

template <int QT>
static void vs_run(const float *logA, const float *logpi, const float *logE, const VsPlan &v, char *ws, int32_t *path,
                   double *score, hipStream_t st) {
    MqModel *mq = (MqModel *)(ws + v.o_mq);
    VsModel *models = (VsModel *)(ws + v.o_model);
    int *vops = (int *)(ws + v.o_vops), *vrb = (int *)(ws + v.o_vrb), *dstart = (int *)(ws + v.o_dstart);
    long long *vmb = (long long *)(ws + v.o_vmb);
    int *sfinal = (int *)(ws + v.o_sfinal);
    const int q = v.q, C = v.C, G = v.G, gs = v.gsize, NB = v.NB;
    const dim3 chains((unsigned)v.nchains), wave(64);
    const bool two = G > 0 && opt(HMM_OPT_SCAN2) != 0;
    const unsigned ngrp = (unsigned)((long long)NB * (two ? G : 1));
    hipLaunchKernelGGL(k_mq_prep, dim3(v.k), wave, 0, st, logA, mq, q, opt(HMM_OPT_FORCE_DENSE) == 1 ? 1 : 0);
    hipLaunchKernelGGL(k_vs_prep, dim3(v.k), wave, 0, st, logA, logpi, models, q);
    const MqModel *cmq = mq;
    const VsModel *cm = models;
    hipLaunchKernelGGL(k_vs_reduce<QT>, chains, wave, 0, st, logE, cmq, cm, vops, vrb, vmb, v);
    if (!two) {
        hipLaunchKernelGGL((k_vs_scan<QT, false>), dim3(NB), wave, 0, st, (const int *)vops, (const int *)vrb,
                           (const long long *)vmb, dstart, (const int *)nullptr, sfinal, score, q, C, 0, 0, 1, (int *)nullptr, 0);
    } else {
        int *gvops = (int *)(ws + v.o_gvops), *gvrb = (int *)(ws + v.o_gvrb), *gdstart = (int *)(ws + v.o_gdstart);
        long long *gvmb = (long long *)(ws + v.o_gvmb);
        hipLaunchKernelGGL((k_vs_compose<QT, false>), dim3(ngrp), wave, 0, st, (const int *)vops, (const int *)vrb,
                           (const long long *)vmb, gvops, gvrb, gvmb, q, C, G, gs);
        hipLaunchKernelGGL((k_vs_scan<QT, false>), dim3(NB), wave, 0, st, (const int *)gvops, (const int *)gvrb,
                           (const long long *)gvmb, gdstart, (const int *)nullptr, sfinal, score, q, G, 0, 0, 1, (int *)nullptr, 0);
        hipLaunchKernelGGL((k_vs_scan<QT, false>), dim3(ngrp), wave, 0, st, (const int *)vops, (const int *)vrb,
                           (const long long *)vmb, dstart, (const int *)gdstart, sfinal, score, q, C, G, gs, 1, (int *)nullptr, 0);
    }
    vs_launch_apply<QT>(logE, v, ws, st);
    if (two) vs_launch_group_maps(v, ws, st);
    vs_launch_backward(v, ws, path, two, st);
}

extern "C" int hmm_viterbi_scan_max_states(void) { return MQ_MAX; }

extern "C" int hmm_viterbi_scan_chunk_len(int k, int b, int L, int q) {
    VsPlan v;
    return make_vsplan(k, b, L, q, &v) ? 0 : v.T;
}

extern "C" size_t hmm_viterbi_scan_workspace_bytes(int k, int b, int L, int q) {
    VsPlan v;
    return make_vsplan(k, b, L, q, &v) ? 0 : v.total;
}

// Where the scan beats hmm_viterbi's one-wave-per-sequence walk (DESIGN 6c, tools/experiments/vit_scan_time.py).
extern "C" int hmm_viterbi_scan_pays(int k, int b, int L, int q) {
    if (k < 1 || b < 1 || L < 1 || q <= QP || q > MQ_MAX) return 0;
    return 0;
}

extern "C" int hmm_viterbi_scan(const float *logA, const float *logpi, const float *logE, int k, int b, int L, int q,
                                int32_t *path, double *score, void *workspace, size_t workspace_bytes, void *stream) {
    if (k < 1 || b < 1 || L < 1 || q < 1) return HMM_ERR_BAD_SHAPE;
    if (q > MQ_MAX) return HMM_ERR_Q_UNSUPPORTED;
    VsPlan v;
    const int rc = make_vsplan(k, b, L, q, &v);
    if (rc) return rc;
    if (!logA || !logpi || !logE || !path || !score || !workspace) return HMM_ERR_NULL_POINTER;
    if (workspace_bytes < v.total || ((uintptr_t)workspace & 255)) return HMM_ERR_WORKSPACE;
    if (v.QT == 32) vs_run<32>(logA, logpi, logE, v, (char *)workspace, path, score, (hipStream_t)stream);
    else vs_run<64>(logA, logpi, logE, v, (char *)workspace, path, score, (hipStream_t)stream);
    return check_launch();
}
