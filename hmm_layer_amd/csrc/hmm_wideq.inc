// hmm_wideq.inc — posteriors and fused posterior decoding for 65 <= q <= 256 states by a per-sequence walk
// (hmm_posterior_walk, hmm_posterior_decode_wide), included by hmm_engine.hip after hmm_midq.inc.
//
// hmm_posterior serves this range with one GEMM launch per position and direction (hmm_largeq.inc), which for a
// 71-state gene model whose states have at most 6 predecessors is all launch latency.  Here ONE workgroup walks one
// sequence, serial in time, with the cell's exact step (max(E, eps), max(pi, eps), the forward clamp of the predicted
// mixture, the backward max(A r, eps), normaliser logs summed in fp64; zero entries of A are exact zeros).  There is
// no certificate and no routing.
//
// Layout (that of k_mq_posterior2, widened): the workgroup is two GROUPS of NP = 64 ceil(q/64) threads, lane = state.
// Group 0 walks forward from t = 0, group 1 backward from t = L - 1, one position per step each, in lockstep.  Until
// they meet at h = ceil(L/2) each parks its vector in `out` (forward: U_t = max(E_t,eps) max(R_t,eps), unnormalised —
// gamma is scale-free in it; backward: Rb_t); afterwards each multiplies its vector into what the other parked and
// writes gamma_t over it.  The current vector of each group lives in LDS, double-buffered, and a step has ONE
// barrier: the wave sums a step needs (the normaliser S_t, the row sum of gamma, the hub sums below) are published
// per wave before the barrier and added in wave order by every lane after it, so a step works with the sums of the
// step before: the vector is carried unnormalised next to 1 / S, gamma_t is formed one step after its position
// (g = U_t Rb_t, once the other group's parked vector is certainly visible) and leaves two steps after it (g / sum g).
//
// Step (STEP), chosen per model on the device by k_wq_prep, no host round trip:
//   0  sparse   every state has at most 8 non-zero predecessors and at most 8 non-zero successors, except at most
//               WQ_HUBS = 2 HUB states of any degree (the intergenic state of a c-copy gene model has c + 1 of each).
//               Lane j keeps its 8 (index, weight) pairs in registers and gathers from the LDS vector; a hub's sum is
//               formed by the whole group: every lane holds its one entry into (forward) or out of (backward) the hub,
//               and the products are summed like the normaliser, wave sums then waves in order.
//   1  dense, q <= 128   lane j keeps column j (forward) or row j (backward) of A in registers (128 VGPRs) and reads
//               the vector from LDS as broadcast 16-byte reads: four accumulators, states in increasing index.
//   2  dense, 129..256   the same sums with A read from global memory every step (forward: A, backward: its
//               transpose made once per call, both L2-resident).  SLOW — q loads per lane and position — and correct;
//               it is what a model outside the sparse rule gets in this range, never something else silently.
// HMM_OPT_FORCE_DENSE = 1 forces the dense step.
//
// Output policy (DEC): NoDecode writes the gamma rows per `mode`; DecodeWide (hmm_posterior_decode_wide) stages the
// finished rows of each group in LDS, WQ_T rows per group, and collapses them with the rules of collapse_row
// (hmm_midq.inc): the class posterior is the fp32 sum over ALL states in increasing index with weights 0 / 1
// (fma(v, 1, s) = s + v rounded once, fma(v, 0, s) = s), classes are compared in increasing index with a strict >,
// and with the identity map nothing is summed.  The class table travels by value as 16 masks of 256 bits.
// ClassWide (hmm_class_posterior_walk) is DecodeWide without the argmax: same staging, masks and class-sum loop (so the
// sums have the bits DecodeWide compares), and drain() writes the ncls sums of every staged row to out_prob and / or
// out_log, where k_wq_class_log turns them into their logs after the walk (a sum of 0 gives -inf).

#define WQ_MIN 65
#define WQ_MAX 256
#define WQ_REG 128               // largest q whose dense step keeps A in registers
#define WQ_SP_MAX 8
#define WQ_HUBS 2
#define WQ_T 16                  // gamma rows each group stages before a collapse (DecodeWide)
#define WQ_PF 8                  // emission rows in flight

struct WqSp {
    int sparse, nhub, hub[WQ_HUBS];          // hub[h] = -1: none
    int fsrc[WQ_MAX][WQ_SP_MAX];             // predecessors of state j, pads: 0 with weight 0 (hubs: all pads)
    float fw[WQ_MAX][WQ_SP_MAX];
    int bsrc[WQ_MAX][WQ_SP_MAX];             // successors of state i
    float bw[WQ_MAX][WQ_SP_MAX];
    float hin[WQ_HUBS][WQ_MAX];              // A[i][hub]: lane i's entry into the hub (forward)
    float hout[WQ_HUBS][WQ_MAX];             // A[hub][j]: lane j's entry out of the hub (backward)
};

struct alignas(8) DecodeWide {
    static constexpr bool on = true;
    static constexpr bool sums = false;         // the argmax leaves, not the sums
    unsigned long long mask[QP][WQ_MAX / 64];   // bit s of mask[c]: state s belongs to class c
    unsigned char *label;                       // (k,b,L)
    float *conf;                                // (k,b,L) or null
    int ncls;                                   // number of classes; 0: the identity map (no sums)
};

struct alignas(8) ClassWide {
    static constexpr bool on = true;
    static constexpr bool sums = true;
    unsigned long long mask[QP][WQ_MAX / 64];   // as DecodeWide's
    float *prob;                                // (k,b,L,ncls) or null
    float *logp;                                // (k,b,L,ncls) or null
    int ncls;                                   // 1 .. QP
};

// one block of 256 threads per model: the lists, the hubs and the verdict
__global__ __launch_bounds__(WQ_MAX) void k_wq_prep(const float *__restrict__ A, WqSp *__restrict__ sp, int q,
                                                    int force_dense) {
    __shared__ int deg[WQ_MAX];
    __shared__ int shub[WQ_HUBS], snh;
    const int m = blockIdx.x, j = threadIdx.x;
    const float *Am = A + (size_t)m * q * q;
    WqSp &M = sp[m];
    int nf = 0, nb = 0;
    if (j < q) {
        for (int i = 0; i < q; ++i) {
            const float a = Am[(size_t)i * q + j];
            if (a != 0.f) { if (nf < WQ_SP_MAX) { M.fsrc[j][nf] = i; M.fw[j][nf] = a; } ++nf; }
            const float c = Am[(size_t)j * q + i];
            if (c != 0.f) { if (nb < WQ_SP_MAX) { M.bsrc[j][nb] = i; M.bw[j][nb] = c; } ++nb; }
        }
    }
    deg[j] = nf > nb ? nf : nb;
    __syncthreads();
    if (j == 0) {
        int n = 0;
        shub[0] = shub[1] = -1;
        for (int s = 0; s < q; ++s)
            if (deg[s] > WQ_SP_MAX) { if (n < WQ_HUBS) shub[n] = s; ++n; }
        snh = n;
    }
    __syncthreads();
    const int h0 = shub[0], h1 = shub[1];
    if (j == h0 || j == h1) nf = nb = 0;                     // a hub's sums come from the whole group
    for (int e = nf < WQ_SP_MAX ? nf : WQ_SP_MAX; e < WQ_SP_MAX; ++e) { M.fsrc[j][e] = 0; M.fw[j][e] = 0.f; }
    for (int e = nb < WQ_SP_MAX ? nb : WQ_SP_MAX; e < WQ_SP_MAX; ++e) { M.bsrc[j][e] = 0; M.bw[j][e] = 0.f; }
    M.hin[0][j] = (h0 >= 0 && j < q) ? Am[(size_t)j * q + h0] : 0.f;
    M.hin[1][j] = (h1 >= 0 && j < q) ? Am[(size_t)j * q + h1] : 0.f;
    M.hout[0][j] = (h0 >= 0 && j < q) ? Am[(size_t)h0 * q + j] : 0.f;
    M.hout[1][j] = (h1 >= 0 && j < q) ? Am[(size_t)h1 * q + j] : 0.f;
    if (j == 0) {
        const int ok = !force_dense && snh <= WQ_HUBS;
        M.sparse = ok;
        M.nhub = ok ? snh : 0;
        M.hub[0] = h0; M.hub[1] = h1;
    }
}

// dynamic LDS of the decode form: the masks, the two groups' rings (rows q | 1 floats apart), the class sums
static unsigned wq_decode_lds(int q) {
    return (unsigned)(QP * (WQ_MAX / 64) * sizeof(unsigned long long) + (2 * WQ_T * (q | 1) + 2 * WQ_T * QP) * sizeof(float));
}

// A: (k,q,q); At: its transpose (STEP 2 only, else unused); out: the output tensor, or DecodeWide's parking region
template <int STEP, class DEC>
__device__ __forceinline__ void wq_walk_body(const float *__restrict__ A, const float *__restrict__ At,
                                             const float *__restrict__ pi, const float *__restrict__ E, int b, int L,
                                             int q, float eps, float *__restrict__ out, double *__restrict__ ll, int mode,
                                             const WqSp *__restrict__ sp, const DEC &dec, unsigned long long *dyn) {
    __shared__ __attribute__((aligned(16))) float xs[2][2][WQ_MAX];   // [group][buffer][state]
    __shared__ f4 part[2][2][4];                                      // [buffer][group][wave]: S, sum g, hub 0, hub 1
    __shared__ double llsh;
    const long long row = blockIdx.x;
    const int m = (int)(row / b);
    const WqSp &M = sp[m];
    if ((M.sparse != 0) != (STEP == 0)) return;              // block-uniform, before any barrier: the other form has it
    const int NP = blockDim.x >> 1;
    const int dir = __builtin_amdgcn_readfirstlane(threadIdx.x >= NP ? 1 : 0);   // 0: forward group, 1: backward group
    const int j = threadIdx.x - dir * NP, lane = j & 63, w = j >> 6, nw = NP >> 6;
    const bool act = j < q;
    const int jc = act ? j : q - 1;
    const float *Am = A + (size_t)m * q * q;
    const float *Er = E + (size_t)row * L * q;
    float *o = out + (size_t)row * L * q;
    const int h = (L + 1) / 2;

    // ---- this lane's coefficients
    i4 s0 = {0, 0, 0, 0}, s1 = {0, 0, 0, 0};
    f4 w0 = {0.f, 0.f, 0.f, 0.f}, w1 = {0.f, 0.f, 0.f, 0.f};
    float hw0 = 0.f, hw1 = 0.f;
    int hub0 = -1, hub1 = -1, nhub = 0;
    constexpr int NA = STEP == 1 ? WQ_REG : 4;
    float av[NA];
    const float *Ag = nullptr;
    if constexpr (STEP == 0) {
        const int (*src)[WQ_SP_MAX] = dir ? M.bsrc : M.fsrc;
        const float (*wt)[WQ_SP_MAX] = dir ? M.bw : M.fw;
        s0 = *reinterpret_cast<const i4 *>(&src[j][0]); s1 = *reinterpret_cast<const i4 *>(&src[j][4]);
        w0 = *reinterpret_cast<const f4 *>(&wt[j][0]);  w1 = *reinterpret_cast<const f4 *>(&wt[j][4]);
        nhub = M.nhub; hub0 = M.hub[0]; hub1 = M.hub[1];
        hw0 = dir ? M.hout[0][j] : M.hin[0][j];
        hw1 = dir ? M.hout[1][j] : M.hin[1][j];
    } else if constexpr (STEP == 1) {
#pragma unroll
        for (int i = 0; i < NA; ++i)
            av[i] = (act && i < q) ? (dir ? Am[(size_t)j * q + i] : Am[(size_t)i * q + j]) : 0.f;
    } else {
        Ag = (dir ? At + (size_t)m * q * q : Am) + jc;      // forward: column j of A; backward: column j of A^T = row j
    }
    auto matvec = [&](const float *xv) -> float {
        if constexpr (STEP == 0) {
            float r = fmaf(w0.w, xv[s0.w], fmaf(w0.z, xv[s0.z], fmaf(w0.y, xv[s0.y], w0.x * xv[s0.x])));
            r += fmaf(w1.w, xv[s1.w], fmaf(w1.z, xv[s1.z], fmaf(w1.y, xv[s1.y], w1.x * xv[s1.x])));
            return r;
        } else if constexpr (STEP == 1) {
            float a[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int i = 0; i < NA; i += 4) {
                const f4 x = *reinterpret_cast<const f4 *>(xv + i);
                a[0] = fmaf(x.x, av[i], a[0]);
                a[1] = fmaf(x.y, av[i + 1], a[1]);
                a[2] = fmaf(x.z, av[i + 2], a[2]);
                a[3] = fmaf(x.w, av[i + 3], a[3]);
            }
            return (a[0] + a[1]) + (a[2] + a[3]);
        } else {
            float a[4] = {0.f, 0.f, 0.f, 0.f};
            const int q4 = q & ~3;
#pragma unroll 2
            for (int i = 0; i < q4; i += 4) {
                const f4 x = *reinterpret_cast<const f4 *>(xv + i);
                a[0] = fmaf(x.x, Ag[(size_t)i * q], a[0]);
                a[1] = fmaf(x.y, Ag[(size_t)(i + 1) * q], a[1]);
                a[2] = fmaf(x.z, Ag[(size_t)(i + 2) * q], a[2]);
                a[3] = fmaf(x.w, Ag[(size_t)(i + 3) * q], a[3]);
            }
            for (int i = q4; i < q; ++i) a[i & 3] = fmaf(xv[i], Ag[(size_t)i * q], a[i & 3]);
            return (a[0] + a[1]) + (a[2] + a[3]);
        }
    };

    // ---- DecodeWide: masks, rings and class sums in dynamic LDS; the counters are block-uniform (every thread keeps
    // both groups')
    unsigned long long *lmask = dyn;
    const int rs = q | 1;
    float *ring = reinterpret_cast<float *>(dyn + QP * (WQ_MAX / 64));
    float *csum = ring + 2 * WQ_T * rs;
    int cntF = 0, cntB = 0, firstF = 0, firstB = 0;
    if constexpr (DEC::on) {
#pragma unroll
        for (int c = 0; c < QP; ++c)                         // (constant indices: the masks stay arguments)
#pragma unroll
            for (int u = 0; u < WQ_MAX / 64; ++u)
                if ((int)threadIdx.x == c * (WQ_MAX / 64) + u) lmask[c * (WQ_MAX / 64) + u] = dec.mask[c][u];
        __syncthreads();
    }
    auto drain = [&]() {                                     // called by the whole block
        if constexpr (DEC::on) {
            const int nrows = cntF + cntB, ncls = dec.ncls;
            if (ncls > 0) {
                for (int p = threadIdx.x; p < nrows * ncls; p += blockDim.x) {
                    const int rr = p / ncls, c = p - rr * ncls;
                    const int slot = rr < cntF ? rr : WQ_T + rr - cntF;
                    const float *rp = ring + slot * rs;
                    float sum = 0.f;                                       // ALL states in increasing index
                    for (int u = 0; u < WQ_MAX / 64; ++u) {
                        const unsigned long long mk = lmask[c * (WQ_MAX / 64) + u];
                        const int n = q - 64 * u < 64 ? q - 64 * u : 64;
                        for (int s = 0; s < n; ++s)
                            sum = __builtin_fmaf(rp[64 * u + s], ((mk >> s) & 1ull) ? 1.f : 0.f, sum);
                    }
                    csum[slot * QP + c] = sum;
                }
                __syncthreads();
            }
            if constexpr (DEC::sums) {                      // ClassWide: the sums themselves (ncls >= 1)
                for (int p = threadIdx.x; p < nrows * ncls; p += blockDim.x) {
                    const int rr = p / ncls, c = p - rr * ncls;
                    const int slot = rr < cntF ? rr : WQ_T + rr - cntF;
                    const int t = rr < cntF ? firstF + rr : firstB - (rr - cntF);
                    const float v = csum[slot * QP + c];
                    const size_t at = ((size_t)row * L + t) * ncls + c;
                    if (dec.prob) dec.prob[at] = v;
                    if (dec.logp) dec.logp[at] = v;               // k_wq_class_log takes the log in place, after the walk
                }
            } else {
                for (int rr = threadIdx.x; rr < nrows; rr += blockDim.x) {
                    const int slot = rr < cntF ? rr : WQ_T + rr - cntF;
                    const int t = rr < cntF ? firstF + rr : firstB - (rr - cntF);
                    const float *rp = ncls > 0 ? csum + slot * QP : ring + slot * rs;
                    const int n = ncls > 0 ? ncls : q;
                    float best = rp[0];
                    int lab = 0;
                    for (int s = 1; s < n; ++s) {
                        const float v = rp[s];
                        if (v > best) { best = v; lab = s; }              // strict: the lowest index wins a tie
                    }
                    const long long at = row * L + t;
                    dec.label[at] = (unsigned char)lab;
                    if (dec.conf) dec.conf[at] = best;
                }
            }
            __syncthreads();
            cntF = cntB = 0;
        }
    };

    // ---- the walk: L + 2 steps (the last two only finish the positions of the two steps before)
    double lacc = 0.0;
    float vprev = 0.f, g2 = 0.f;
    auto step = [&](const int s, const int sb, const float eraw, const float ppre) {
        const int t = dir ? L - 1 - s : s;                    // this step's position (s < L)
        const int tp = dir ? t + 1 : t - 1, tpp = dir ? t + 2 : t - 2;   // ... of the step before, and two before
        const bool comb1 = s >= 1 && s - 1 < L && (dir ? tp < h : tp >= h);
        const bool emit2 = s >= 2 && s - 2 < L && (dir ? tpp < h : tpp >= h);
        if constexpr (DEC::on) {
            if (cntF == WQ_T || cntB == WQ_T) drain();
        }
        // what the other group parked at tp: it wrote that in its step wstep.  Where that lies before the step in which
        // this block of steps was requested (rows), the prefetched value is the parked one; around the meeting point
        // it is read here, a barrier or more after it was written.
        float pk = ppre;
        if (comb1 && !((dir ? tp : L - 1 - tp) < sb - WQ_PF)) pk = o[(size_t)tp * q + jc];
        float Sp = 1.f, Sg = 1.f, hs0 = 0.f, hs1 = 0.f;
        if (s > 0) {
            f4 a = part[(s - 1) & 1][dir][0];
            for (int x = 1; x < nw; ++x) a += part[(s - 1) & 1][dir][x];   // waves in order
            Sp = a.x; Sg = a.y; hs0 = a.z; hs1 = a.w;
        }
        if (emit2) {
            const float gam = g2 * __builtin_amdgcn_rcpf(Sg);
            if constexpr (DEC::on) {
                if (act) ring[((dir ? WQ_T : 0) + (dir ? cntB : cntF)) * rs + j] = gam;
            } else {
                const float v = mode == 0 ? gam : __logf(g2) - __logf(Sg);
                if (act) o[(size_t)tpp * q + j] = v;
            }
        }
        if constexpr (DEC::on) {                              // both groups' counters, in every thread
            if (s >= 2 && s - 2 < L) {
                if (s - 2 >= h) { if (cntF == 0) firstF = s - 2; ++cntF; }
                if (L - 1 - (s - 2) < h) { if (cntB == 0) firstB = L - 1 - (s - 2); ++cntB; }
            }
        }
        if (!dir && s >= 1 && s <= L) lacc += (double)logf(Sp);
        float sf = 0.f, val = 0.f;
        if (s < L) {
            float rc;
            if (s == 0) {
                rc = dir ? 1.f : fmaxf(pi[(size_t)m * q + jc], eps);
            } else {
                float r = matvec(xs[dir][(s - 1) & 1]);
                if constexpr (STEP == 0) r = j == hub0 ? hs0 : (j == hub1 ? hs1 : r);
                rc = fmaxf(r * __builtin_amdgcn_rcpf(Sp), eps);
            }
            sf = act ? fmaxf(eraw, eps) * rc : 0.f;
            val = act ? (dir ? rc : sf) : 0.f;
            xs[dir][s & 1][j] = sf;
            if (!(dir ? t < h : t >= h) && act) o[(size_t)t * q + j] = val;      // park
        }
        const float g1 = comb1 ? vprev * pk : 0.f;
        f4 ps;
        ps.x = mq_wave_sum(sf);
        ps.y = mq_wave_sum(g1);
        ps.z = 0.f; ps.w = 0.f;
        if constexpr (STEP == 0) {
            if (nhub > 0) ps.z = mq_wave_sum(sf * hw0);
            if (nhub > 1) ps.w = mq_wave_sum(sf * hw1);
        }
        if (lane == 0) part[s & 1][dir][w] = ps;
        g2 = g1; vprev = val;
        __syncthreads();
    };
    // emission rows, and the rows of `out` the steps combine with, WQ_PF steps ahead; positions outside the sequence
    // re-read a valid row (no branch around the loads)
    auto rows = [&](int sb, float (&r)[WQ_PF], float (&pr)[WQ_PF]) {
#pragma unroll
        for (int u = 0; u < WQ_PF; ++u) {
            const int s = sb + u < L ? sb + u : L - 1;
            r[u] = Er[(size_t)(dir ? L - 1 - s : s) * q + jc];
            int tp = dir ? L - (sb + u) : sb + u - 1;          // the position of step sb + u - 1
            tp = tp < 0 ? 0 : (tp > L - 1 ? L - 1 : tp);
            pr[u] = o[(size_t)tp * q + jc];
        }
    };
    float en[WQ_PF], pn[WQ_PF];
    rows(0, en, pn);
    for (int sb = 0; sb < L + 2; sb += WQ_PF) {
        float cur[WQ_PF], cp[WQ_PF];
#pragma unroll
        for (int u = 0; u < WQ_PF; ++u) { cur[u] = en[u]; cp[u] = pn[u]; }
        rows(sb + WQ_PF, en, pn);
#pragma unroll
        for (int u = 0; u < WQ_PF; ++u)
            if (sb + u < L + 2) step(sb + u, sb, cur[u], cp[u]);   // block-uniform
    }
    drain();
    if (!dir && j == 0) {
        ll[row] = lacc;
        llsh = lacc;
    }
    if constexpr (!DEC::on) {
        if (mode == 2) {                                     // log gamma + loglik: the forward group knows it only now
            __syncthreads();
            const double l = llsh;
            const size_t n = (size_t)L * q;
            for (size_t i = threadIdx.x; i < n; i += blockDim.x) o[i] = (float)((double)o[i] + l);
        }
    }
}

template <int STEP>
__global__ __launch_bounds__(STEP == 1 ? 2 * WQ_REG : 2 * WQ_MAX)
void k_wq_walk(const float *__restrict__ A, const float *__restrict__ At, const float *__restrict__ pi,
               const float *__restrict__ E, int b, int L, int q, float eps, float *__restrict__ out,
               double *__restrict__ ll, int mode, const WqSp *__restrict__ sp) {
    wq_walk_body<STEP, NoDecode>(A, At, pi, E, b, L, q, eps, out, ll, mode, sp, NoDecode(), nullptr);
}

// the DecodeWide form; park: the workspace's parking region.  Dynamic LDS: wq_decode_lds(q) bytes.
template <int STEP>
__global__ __launch_bounds__(STEP == 1 ? 2 * WQ_REG : 2 * WQ_MAX)
void k_wq_walk_decode(const float *__restrict__ A, const float *__restrict__ At, const float *__restrict__ pi,
                      const float *__restrict__ E, int b, int L, int q, float eps, float *__restrict__ park,
                      double *__restrict__ ll, const WqSp *__restrict__ sp, const DecodeWide dec) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long wq_lds[];
    wq_walk_body<STEP, DecodeWide>(A, At, pi, E, b, L, q, eps, park, ll, 0, sp, dec, wq_lds);
}

// the ClassWide form; park and dynamic LDS as for k_wq_walk_decode
template <int STEP>
__global__ __launch_bounds__(STEP == 1 ? 2 * WQ_REG : 2 * WQ_MAX)
void k_wq_walk_class(const float *__restrict__ A, const float *__restrict__ At, const float *__restrict__ pi,
                     const float *__restrict__ E, int b, int L, int q, float eps, float *__restrict__ park,
                     double *__restrict__ ll, const WqSp *__restrict__ sp, const ClassWide dec) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long wq_lds[];
    wq_walk_body<STEP, ClassWide>(A, At, pi, E, b, L, q, eps, park, ll, 0, sp, dec, wq_lds);
}

// out_log of the ClassWide form, in place: the sums the walk left there -> their logs, -inf for 0.  The fp64 log rounded
// once: logf measured 2.04 ulp on these sums, over the 2 ulp the header promises, and the fp64 log inside drain() cost
// the sparse walk 30 VGPRs and one of its two workgroups per CU.  n = k b L ncls elements, grid-stride.
__global__ __launch_bounds__(256) void k_wq_class_log(float *__restrict__ x, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        x[i] = (float)log((double)x[i]);
}

// ---- host side
struct WqPlan { size_t o_ll, o_sp, o_At, total; };
static int make_wqplan(int k, int b, int L, int q, WqPlan *p) {
    if (k < 1 || b < 1 || L < 1 || q < 1) return HMM_ERR_BAD_SHAPE;
    if (q < WQ_MIN || q > WQ_MAX) return HMM_ERR_Q_UNSUPPORTED;
    size_t off = 0;
    p->o_ll = off; off = align_up(off + (size_t)k * b * sizeof(double));
    p->o_sp = off; off = align_up(off + (size_t)k * sizeof(WqSp));
    p->o_At = off; off = align_up(off + (q > WQ_REG ? (size_t)k * q * q * sizeof(float) : 0));   // STEP 2 reads A^T
    p->total = off;
    return HMM_OK;
}

// dec and cls null: gamma rows per `mode` into `out`; dec: labels, cls: class sums, with `out` the parking region
static void wq_walk(const float *A, const float *pi, const float *E, int k, int b, int L, int q, float eps, int mode,
                    float *out, const WqPlan &p, char *ws, const DecodeWide *dec, hipStream_t st,
                    const ClassWide *cls = nullptr) {
    WqSp *sp = ws_at<WqSp>(ws, p.o_sp);
    const WqSp *csp = sp;
    double *ll = ws_at<double>(ws, p.o_ll);
    float *At = ws_at<float>(ws, p.o_At);
    launch(k_wq_prep, dim3(k), dim3(WQ_MAX), 0, st, A, sp, q, opt(HMM_OPT_FORCE_DENSE) == 1 ? 1 : 0);
    if (q > WQ_REG) launch(k_lq_transpose, dim3((q + 31) / 32, (q + 31) / 32, k), dim3(256), 0, st, A, At, q);
    const dim3 grid((unsigned)((size_t)k * b)), blk((unsigned)(2 * ((q + 63) / 64 * 64)));
    const float *cAt = At;
    if (cls) {
        const unsigned lds = wq_decode_lds(q);
        launch(k_wq_walk_class<0>, grid, blk, lds, st, A, cAt, pi, E, b, L, q, eps, out, ll, csp, *cls);
        launch(q <= WQ_REG ? k_wq_walk_class<1> : k_wq_walk_class<2>, grid, blk, lds, st, A, cAt, pi, E, b, L, q, eps,
               out, ll, csp, *cls);
    } else if (dec) {
        const unsigned lds = wq_decode_lds(q);
        launch(k_wq_walk_decode<0>, grid, blk, lds, st, A, cAt, pi, E, b, L, q, eps, out, ll, csp, *dec);
        launch(q <= WQ_REG ? k_wq_walk_decode<1> : k_wq_walk_decode<2>, grid, blk, lds, st, A, cAt, pi, E, b, L, q, eps,
               out, ll, csp, *dec);
    } else {
        launch(k_wq_walk<0>, grid, blk, 0, st, A, cAt, pi, E, b, L, q, eps, out, ll, mode, csp);
        launch(q <= WQ_REG ? k_wq_walk<1> : k_wq_walk<2>, grid, blk, 0, st, A, cAt, pi, E, b, L, q, eps, out, ll, mode,
               csp);
    }
}

extern "C" {

int hmm_posterior_walk_min_states(void) { return WQ_MIN; }
int hmm_posterior_walk_max_states(void) { return WQ_MAX; }

size_t hmm_posterior_walk_workspace_bytes(int k, int b, int L, int q) {
    WqPlan p;
    return make_wqplan(k, b, L, q, &p) ? 0 : p.total;
}

// 1 where the fused decode measured at least 1.25x faster than hmm_posterior + a reduction (DESIGN, "Decoded output,
// 65-256 states"; tools/experiments/posterior_walk_time.py, profiles/posterior_walk.json); 0 where nothing was
// measured.  Measured on one MI355X at L = 10 000, one model, 1 / 32 / 1024 sequences: the sparse step at 71, 127 and
// 253 states 9.2 .. 14.0x, the dense step at 96 and 128 states 2.9 .. 8.9x — every cell pays, so the rule is the
// measured range itself: up to WQ_PAYS_SEQS sequences in the call (the walk's cost goes with the number of sequences,
// the GEMMs' with launches per model).  More sequences were not measured.  L does not enter: both evaluations cost
// per position (2 L launches against L steps).  Above 128 states only the sparse step was measured, and only models
// that take it should be sent here (engine.posterior_decode's `sparse`).
#define WQ_PAYS_SEQS 1024
int hmm_posterior_walk_pays(int k, int b, int L, int q) {
    WqPlan p;
    if (make_wqplan(k, b, L, q, &p)) return 0;
    return (long long)k * b <= WQ_PAYS_SEQS ? 1 : 0;
}

int hmm_posterior_walk(const float *A, const float *pi, const float *E, int k, int b, int L, int q, float eps, int mode,
                       float *out, double *loglik, void *workspace, size_t workspace_bytes, void *stream) {
    WqPlan p;
    int rc = make_wqplan(k, b, L, q, &p);
    if (rc) return rc;
    if (!A || !pi || !E || !out || !workspace) return HMM_ERR_NULL_POINTER;
    if (mode < HMM_POST_PROB || mode > HMM_POST_LOG_NO_LL || check_eps(eps)) return HMM_ERR_BAD_ARGUMENT;
    if ((rc = check_ws(p.total, workspace, workspace_bytes))) return rc;
    hipStream_t st = (hipStream_t)stream;
    wq_walk(A, pi, E, k, b, L, q, eps, mode, out, p, (char *)workspace, nullptr, st);
    if (loglik) launch(k_copy_loglik, dim3((k * b + 255) / 256), dim3(256), 0, st, ws_at<double>(workspace, p.o_ll), loglik, k * b);
    return check_launch();
}

size_t hmm_posterior_decode_wide_workspace_bytes(int k, int b, int L, int q) {
    WqPlan p;
    if (make_wqplan(k, b, L, q, &p)) return 0;
    return align_up(p.total) + (size_t)k * b * L * q * sizeof(float);
}

int hmm_posterior_decode_wide(const float *A, const float *pi, const float *E, int k, int b, int L, int q, float eps,
                              const int *state_class, int num_classes, unsigned char *label, float *conf,
                              double *loglik, void *workspace, size_t workspace_bytes, void *stream) {
    WqPlan p;
    int rc = make_wqplan(k, b, L, q, &p);
    if (rc) return rc;
    if (!A || !pi || !E || !label || !workspace) return HMM_ERR_NULL_POINTER;
    if (num_classes < 1 || (state_class ? num_classes > QP : num_classes != q) || check_eps(eps)) return HMM_ERR_BAD_ARGUMENT;
    DecodeWide dec{};
    dec.label = label; dec.conf = conf; dec.ncls = state_class ? num_classes : 0;
    for (int s = 0; s < q && state_class; ++s) {               // the table is read here, once, and travels by value
        if (state_class[s] < 0 || state_class[s] >= num_classes) return HMM_ERR_BAD_ARGUMENT;
        dec.mask[state_class[s]][s >> 6] |= 1ull << (s & 63);
    }
    const size_t o_park = align_up(p.total);
    if ((rc = check_ws(o_park + (size_t)k * b * L * q * sizeof(float), workspace, workspace_bytes))) return rc;
    hipStream_t st = (hipStream_t)stream;
    wq_walk(A, pi, E, k, b, L, q, eps, HMM_POST_PROB, ws_at<float>(workspace, o_park), p, (char *)workspace, &dec, st);
    if (loglik) launch(k_copy_loglik, dim3((k * b + 255) / 256), dim3(256), 0, st, ws_at<double>(workspace, p.o_ll), loglik, k * b);
    return check_launch();
}

size_t hmm_class_posterior_walk_workspace_bytes(int k, int b, int L, int q) {
    return hmm_posterior_decode_wide_workspace_bytes(k, b, L, q);
}

// 1 where autograd's fused class-posterior node (this forward + hmm_class_posterior_grad_walk) measured at least 1.25x
// faster than the composition it replaces (DESIGN §12f; tools/experiments/class_posterior_walk_time.py,
// profiles/class_posterior_walk.json); 0 where nothing was measured.  Measured on one MI355X at L = 10 000, one model,
// 6 classes, log mode, a label-style upstream gradient, the gene models of 71, 127 and 253 states at 1 / 32 / 1024
// sequences: 0.93 .. 1.00x at 1 and 32 sequences (the walks are latency-bound there, and the class forward costs 1.5 to
// 4 ms more than hmm_posterior_walk), 1.58x / 2.04x / 1.83x at 1024.  So the rule is the three cells that pay and
// nothing else: neither the crossover between 32 and 1024 sequences, nor more than 1024, nor other state counts were
// measured, nor more than one model per call (k > 1: 0).  The one extrapolation is L, by the convention of
// hmm_posterior_walk_pays and hmm_posterior_grad_walk_pays: it does not enter, both evaluations cost per position.
#define CPW_PAYS_SEQS 1024
int hmm_class_posterior_walk_pays(int k, int b, int L, int q) {
    WqPlan p;
    if (make_wqplan(k, b, L, q, &p)) return 0;
    return (q == 71 || q == 127 || q == 253) && k == 1 && b == CPW_PAYS_SEQS ? 1 : 0;
}

int hmm_class_posterior_walk(const float *A, const float *pi, const float *E, int k, int b, int L, int q, float eps,
                             const int *state_class, int num_classes, float *out_prob, float *out_log, double *loglik,
                             void *workspace, size_t workspace_bytes, void *stream) {
    WqPlan p;
    int rc = make_wqplan(k, b, L, q, &p);
    if (rc) return rc;
    if (!A || !pi || !E || !state_class || !workspace || (!out_prob && !out_log)) return HMM_ERR_NULL_POINTER;
    if (num_classes < 1 || num_classes > QP || check_eps(eps)) return HMM_ERR_BAD_ARGUMENT;
    ClassWide cls{};
    cls.prob = out_prob; cls.logp = out_log; cls.ncls = num_classes;
    for (int s = 0; s < q; ++s) {                              // the table is read here, once, and travels by value
        if (state_class[s] < 0 || state_class[s] >= num_classes) return HMM_ERR_BAD_ARGUMENT;
        cls.mask[state_class[s]][s >> 6] |= 1ull << (s & 63);
    }
    const size_t o_park = align_up(p.total);
    if ((rc = check_ws(o_park + (size_t)k * b * L * q * sizeof(float), workspace, workspace_bytes))) return rc;
    hipStream_t st = (hipStream_t)stream;
    wq_walk(A, pi, E, k, b, L, q, eps, HMM_POST_PROB, ws_at<float>(workspace, o_park), p, (char *)workspace, nullptr, st,
            &cls);
    if (out_log) {
        const size_t n = (size_t)k * b * L * num_classes, nb = (n + 255) / 256;
        launch(k_wq_class_log, dim3((unsigned)(nb < 65536 ? nb : 65536)), dim3(256), 0, st, out_log, n);
    }
    if (loglik) launch(k_copy_loglik, dim3((k * b + 255) / 256), dim3(256), 0, st, ws_at<double>(workspace, p.o_ll), loglik, k * b);
    return check_launch();
}

}  // extern "C"
