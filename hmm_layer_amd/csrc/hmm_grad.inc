// Analytic gradient of the sequence log-likelihoods w.r.t. A, pi and E (included by
// hmm_engine.hip).
//
// The reference trains by autograd through the Python time loop (hmm_layer/BaseRNN.py:217-227
// over HmmCell.forward, hmm_layer/MsaHmmCell.py:73-106).  The same derivatives are the
// Baum-Welch expectations, which the posterior pipeline already has in registers:
//
//   d loglik / d E_t[j]  = gamma_t[j] / E_t[j]
//   d loglik / d A[i][j] = sum_t alpha_hat_{t-1}[i] * bh_t[j] / (alpha_hat_{t-1} . A bh_t)      (= sum_t xi_t(i,j) / A[i][j])
//   d loglik / d pi[j]   = gamma_0[j] / pi[j]
//
// with bh_t = normalised(E_t * R_t) the backward vector of the reverse cell.  Entries the cell
// clamps (E or pi below eps) receive no gradient, as torch.maximum routes it to the constant;
// likewise a predicted state (x A)[j] below eps (MsaHmmCell.py:88) passes nothing back: it is
// masked out of the adjoint recursion and of xi_t(., j), which is what decides the gradient of
// absent (zero) edges into dead states.
//
// k_backward_grad is k_backward<0> plus (a) the output is w*gamma/E instead of gamma, and (b) per
// step one 16x16 outer-product sum over the wave's 16 chains, G += P Q^T with
// P = alpha_hat_{t-1} * w / Sg_{t-1}, Q = bh_t.  In the tile layout (state on (g, reg), chain on
// lane & 15) the chains sit on the MFMA's M/N index, never on K, so both factors are transposed
// first, through wave-private LDS (column writes, row reads one step later), and one product accumulates
// G in its D layout (lane (g, j), reg r  <->  G[4g + r][j]).  Round 1 transposed with the matrix pipe
// itself (a product with the identity lands in the transposed operand layout): 12 MFMAs per step instead of
// 4, and the pipe was not as idle as assumed — 8.2 -> 7.5 ms for the whole call without them.
// Per-wave partials are summed in a fixed order in fp64 (deterministic).

#define GR_SLICES 64
#define GR_LD 20                 // LDS row stride of a transposed factor tile
#define GR_TILE (16 * GR_LD)

__device__ __forceinline__ f4 rcp4(f4 v) {
    f4 r = {__builtin_amdgcn_rcpf(v.x), __builtin_amdgcn_rcpf(v.y), __builtin_amdgcn_rcpf(v.z),
            __builtin_amdgcn_rcpf(v.w)};
    return r;
}

// The backward half of one tile: outputs dE = w gamma / E for the tile's positions, G += the xi sums of its
// transitions (D layout), psi += the posterior mass on components the forward cell's clamp made (the loss only
// contains the forward cell).  Rv: the adjoint vector entering at the tile's last position (up to scale); ck + j*ckb:
// alpha_hat entering block j; tps: the wave's LDS slot for the transposed factors (2 * GR_TILE floats, zeroed here).
__device__ __forceinline__ void grad_backward_body(const float *__restrict__ A, const float *__restrict__ E, f4 Rv,
                                                   const float *__restrict__ ck, size_t ckb, float *__restrict__ dE,
                                                   float wch, const Tile &tl, int m, float *seg, float *tps, const Plan &p,
                                                   float eps, f4 &G, float *psi_acc, f4 *Rend) {
    const int lane = threadIdx.x & 63, g = lane >> 4, n = lane & 15;
    const int q = p.q;
    float af[4], ab[4];
    load_A(A + (size_t)m * q * q, q, g, n, af, ab);
    const Bounds bd = make_bounds(g, q, eps);
    const int rowb = q * (int)sizeof(float);
    const OutStage os = make_outstage(seg, reinterpret_cast<char *>(dE + (tl.baseE - E)), q, lane, tl.voff - g * 16, tl.len);
    const f4 zero4 = {0.f, 0.f, 0.f, 0.f};
    float ps = 0.f;
    // one slot of two 16 x 16 tiles per wave, rows GR_LD floats apart (conflict-free column writes, 16-byte
    // aligned row reads); zeroed, so that the very first read-back adds nothing.  (A second slot would push
    // the workgroup past 80 KB of LDS: one workgroup per CU instead of two.)
    for (int i = lane; i < 2 * GR_TILE; i += 64) tps[i] = 0.f;
    __builtin_amdgcn_wave_barrier();

    f4 en[SUB];
    ld_rows<SUB>(tl.rsE, tl.voff + (p.nsub - 1) * SUB * rowb, rowb, en);
    f4 Xn = zero4;
    if (tl.valid && (p.nsub - 1) * SUB < tl.len)
        Xn = *reinterpret_cast<const f4 *>(ck + (size_t)(p.nsub - 1) * ckb);
    for (int j = p.nsub - 1; j >= 0; --j) {
        const int vo = tl.voff + j * SUB * rowb;
        f4 e[SUB];
#pragma unroll
        for (int s = 0; s < SUB; ++s) e[s] = clampE(en[s], bd);
        const f4 Xc = Xn;
        if (j > 0) {
            ld_rows<SUB>(tl.rsE, vo - SUB * rowb, rowb, en);
            if (tl.valid && (j - 1) * SUB < tl.len)
                Xn = *reinterpret_cast<const f4 *>(ck + (size_t)(j - 1) * ckb);
        }
        // recompute alpha_hat for the block.  Where the cell's clamp of the predicted state is
        // active (x A < eps, MsaHmmCell.py:88) autograd passes nothing to A; that flag travels in
        // the (otherwise unused) sign bit of the stored alpha_hat.
        f4 fa[SUB];
        {
            f4 X = Xc;
#pragma unroll
            for (int s = 0; s < SUB; ++s) {
                const bool init = tl.first && j == 0 && s == 0;
                const f4 D = mfma4(af, X);
                const f4 sf = fmax4(sel4(init, X, D), eps) * e[s];
                X = sf * __builtin_amdgcn_rcpf(col_sum(hsum(sf)));
                fa[s].x = D.x > eps ? X.x : -X.x;
                fa[s].y = D.y > eps ? X.y : -X.y;
                fa[s].z = D.z > eps ? X.z : -X.z;
                fa[s].w = D.w > eps ? X.w : -X.w;
            }
        }
        // gamma normaliser of the row about to be emitted; carried from step to step because the
        // xi normaliser of transition (t-1 -> t) is the gamma normaliser of row t-1
        f4 gm = abs4(fa[SUB - 1]) * Rv;
        float inv = __builtin_amdgcn_rcpf(col_sum(hsum(gm)));
#pragma unroll
        for (int s = SUB - 1; s >= 0; --s) {
            const bool act = j * SUB + s < tl.len;
            // posterior mass on components the forward cell's clamp made (the sequence's first row has no prediction)
            if (psi_acc && !(tl.first && j == 0 && s == 0)) ps = fmaf(flagged_dot(fa[s], Rv), act ? inv : 0.f, ps);
            // d loglik / d E: gamma / E, nothing where the cell clamped E (or in padded states).  The sequence's
            // first row keeps w gamma_0 / eps in its clamped entries: dpi = w gamma_0 / pi is read off that row, and
            // a clamped emission takes the gradient from E, not from pi; k_grad_pi zeroes them once it has read them
            const bool row0 = tl.first && j == 0 && s == 0;
            f4 de = gm * (inv * wch) * rcp4(e[s]);
            de.x = (e[s].x > eps || (row0 && 4 * g + 0 < q)) ? de.x : 0.f;
            de.y = (e[s].y > eps || (row0 && 4 * g + 1 < q)) ? de.y : 0.f;
            de.z = (e[s].z > eps || (row0 && 4 * g + 2 < q)) ? de.z : 0.f;
            de.w = (e[s].w > eps || (row0 && 4 * g + 3 < q)) ? de.w : 0.f;
            stage_row(os, n, g, (j % OUT_GB) * SUB + s, de);
            f4 sf = e[s] * Rv;
            float S = col_sum(hsum(sf));
            f4 bh = sf * __builtin_amdgcn_rcpf(S);
            // adjoint of max(x A, eps): nothing flows back through a clamped predicted state
            f4 Q;
            Q.x = __float_as_int(fa[s].x) < 0 ? 0.f : bh.x;
            Q.y = __float_as_int(fa[s].y) < 0 ? 0.f : bh.y;
            Q.z = __float_as_int(fa[s].z) < 0 ? 0.f : bh.z;
            Q.w = __float_as_int(fa[s].w) < 0 ? 0.f : bh.w;
            f4 Rn = fmax4(mfma4(ab, Q), eps);
            // transition (t-1 -> t): alpha_hat_{t-1} is the previous recomputed row, or the block's
            // checkpoint; the sequence's first row has no incoming transition
            const f4 ap = s > 0 ? abs4(fa[s - 1]) : Xc;
            Rv = sel4(act, Rn, Rv);
            const f4 gp = ap * Rv;
            const float invp = __builtin_amdgcn_rcpf(col_sum(hsum(gp)));
            const bool has = act && !(tl.first && j == 0 && s == 0);
            const f4 P = ap * (has ? invp * wch : 0.f);
            // both factors transposed through the wave's LDS slot: the PREVIOUS step's factors are read back
            // (rows), then this step's are written over them (columns; LDS operations of a wave complete in
            // order) — the round trip sits under a whole step's arithmetic; then G += P^T-layout x Q^T-layout
            {
                const f4 PT = *reinterpret_cast<const f4 *>(tps + n * GR_LD + 4 * g);
                const f4 QT = *reinterpret_cast<const f4 *>(tps + GR_TILE + n * GR_LD + 4 * g);
                __builtin_amdgcn_wave_barrier();
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    tps[(4 * g + r) * GR_LD + n] = P[r];
                    tps[GR_TILE + (4 * g + r) * GR_LD + n] = Q[r];
                }
                __builtin_amdgcn_wave_barrier();
                G = mfma4v(PT, QT, G);
            }
            gm = gp; inv = invp;          // row t-1's gamma (recomputed at the block boundary)
        }
        if (j % OUT_GB == 0) {
            const int top = p.nsub - j;
            flush_rows(os, lane, j * SUB, (top < OUT_GB ? top : OUT_GB) * SUB);
        }
    }
    {   // the last step's factors are still in the slot
        const f4 PT = *reinterpret_cast<const f4 *>(tps + n * GR_LD + 4 * g);
        const f4 QT = *reinterpret_cast<const f4 *>(tps + GR_TILE + n * GR_LD + 4 * g);
        G = mfma4v(PT, QT, G);
    }
    if (psi_acc) *psi_acc = col_sum(ps);
    if (Rend) *Rend = Rv;
}

// is chain c of sequence seq left to the serial plan / to a window (verdicts and final window extents)?
__device__ __forceinline__ bool chain_routed(const int *flags, const int *wtab, int seq, int c) {
    const int f = flags[seq];
    if (f == ROUTE_WHOLE) return true;
    if (f != ROUTE_WINDOWS) return false;
    const int *wt = wtab + (size_t)seq * WIN_STRIDE;
    bool in = false;
    for (int i = 0; i < wt[0]; ++i) in = in || (c >= wt[2 + 2 * i] && c < wt[2 + 2 * i] + wt[3 + 2 * i]);
    return in;
}

// EXACT: the serial exact-clamp plan (see k_forward / k_backward in hmm_engine.hip); models routed
// there by k_topo_check are skipped by the scan plan's waves and vice versa.  Every wave of both
// launches owns one slot of `gpart` (model m: scan waves first, then exact waves, then one slot per sequence for
// its windows) and writes it — zeros when it has nothing to do — so the fixed-order sum needs no knowledge of the
// routing.
//
// Per-sequence routing (scan plan).  The loss only contains the FORWARD cell, so what separates its serial
// recursion from the clamp-free chunk scan is the posterior mass of paths born at the forward cell's clamp
// (backward_body's psi, forward flags only); the first launch sums it per chain (psi) and leaves the adjoint vector
// at every chain's first position (rstart), k_exact_select takes the verdict per sequence, the flagged runs of chunks
// are walked serially in windows (k_window_grad: dE of their positions, their share of dA in the sequence's own slot
// of gpart), and a second launch of the scan plan (redo != null) recomputes exactly those waves that hold routed
// chains with these chains left out.  A wave's partial is a sum over its 16 chains inside the matrix product, so it
// cannot be corrected chain by chain after the fact.
template <bool EXACT>
__global__ __launch_bounds__(256) void k_backward_grad(const float *__restrict__ A, const float *__restrict__ E,
                                                       const float *__restrict__ ckpt,
                                                       const float *__restrict__ suffix,
                                                       const float *__restrict__ gw, float *__restrict__ dE,
                                                       float *__restrict__ gpart, Routing rt, long long wpm_this,
                                                       long long slot_base, long long wtot, Plan p, float eps,
                                                       long long nwaves, float *__restrict__ psi = nullptr,
                                                       const int *__restrict__ redo = nullptr,
                                                       const int *__restrict__ wtab = nullptr,
                                                       float *__restrict__ rstart = nullptr) {
    const long long wave = (long long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (wave >= nwaves) return;
    const int lane = threadIdx.x & 63, g = lane >> 4, n = lane & 15;
    const int q = p.q;
    int m; long long wc0;
    Tile tl = make_tile(E, p, wave, g, n, &m, &wc0);
    float *gslot = gpart + (size_t)((long long)m * wtot + slot_base + (wave - (long long)m * wpm_this)) * (QP * QP);
    if (!EXACT && redo) {
        // second launch: only waves that hold routed chains, and without those chains
        const bool routed = tl.valid && chain_routed(redo, wtab, (int)(tl.chain / p.C), (int)(tl.chain % p.C));
        if (__builtin_amdgcn_ballot_w64(routed) == 0ull || rt.topo[m] == TOPO_EXACT) return;
        if (routed) { tl.valid = false; tl.len = 0; }
    }
    if (!route_tile<EXACT>(tl, m, g, rt, eps)) {
#pragma unroll
        for (int r = 0; r < 4; ++r) gslot[(4 * g + r) * QP + n] = 0.f;
        return;
    }
    __shared__ __attribute__((aligned(16))) float ostage[4 * OUT_SEG];
    __shared__ __attribute__((aligned(16))) float tpose[4 * 2 * GR_TILE];
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // (a chain that is left out may have anything in its suffix vector: ones keep its lanes finite)
    const f4 R0 = (EXACT || !tl.valid) ? ones4(q, g) : *reinterpret_cast<const f4 *>(suffix + (size_t)tl.chain * QP + 4 * g);
    const float wch = tl.valid ? (gw ? gw[tl.chain / p.C] : 1.f) : 0.f;     // upstream d(loss)/d(loglik)
    f4 G = {0.f, 0.f, 0.f, 0.f};
    float ps = 0.f;
    f4 re;
    grad_backward_body(A, E, R0, ckpt + ckpt_origin(tl, p, g, n), ckpt_block(p), dE, wch, tl, m, ostage + w * OUT_SEG,
                       tpose + w * (2 * GR_TILE), p, eps, G, (!EXACT && psi) ? &ps : nullptr, &re);
    // per-wave partial of sum_t xi / A, D layout -> row-major 16x16
#pragma unroll
    for (int r = 0; r < 4; ++r) gslot[(4 * g + r) * QP + n] = G[r];
    if (!EXACT && psi && g == 0 && tl.valid) psi[tl.chain] = ps;
    if (!EXACT && rstart && tl.valid) *reinterpret_cast<f4 *>(rstart + (size_t)tl.chain * QP + 4 * g) = re;
}

// The windows of the gradient call (window_walk in hmm_engine.hip): the same forward half as the posterior's, the
// gradient's backward body on the way back; the windows' share of dA goes to the sequence's own slot of gpart.
struct GradWindows {
    static constexpr bool BACKWARD = true, CKPT = true, LOGA = false;
    __device__ __forceinline__ float *loga() const { return nullptr; }
    const float *gw;
    float *dE, *gpart, *tps;
    long long wtot, slot_base;
    int b;
    float wch;
    f4 G;
    __device__ __forceinline__ void begin(int seq, int, float) {
        wch = gw ? gw[seq] : 1.f;
        G = f4{0.f, 0.f, 0.f, 0.f};
    }
    __device__ __forceinline__ void backward(const float *A, const float *E, const Tile &tl, int m, f4 R, const float *ck,
                                             const Plan &pw, float eps, float *seg, f4 *re) {
        // (a column without a window must stay finite: its zero weight still meets the others' factors in G's sum
        // over the 16 columns)
        const f4 Rs = sel4(tl.valid, R, ones4(pw.q, (threadIdx.x & 63) >> 4));
        grad_backward_body(A, E, Rs, ck, (size_t)QP, dE, tl.valid ? wch : 0.f, tl, m, seg, tps, pw, eps, G, nullptr, re);
    }
    __device__ __forceinline__ void finish(int seq, int m, bool good) {
        const int lane = threadIdx.x & 63, g = lane >> 4, n = lane & 15;
        float *gslot = gpart + (size_t)((long long)m * wtot + slot_base + (seq - m * b)) * (QP * QP);
#pragma unroll
        for (int r = 0; r < 4; ++r) gslot[(4 * g + r) * QP + n] = good ? G[r] : 0.f;    // (not good: the serial plan has it)
    }
};

__global__ __launch_bounds__(256) void k_window_grad(const float *__restrict__ A, const float *__restrict__ E,
                                                     const float *__restrict__ prefix, const double *__restrict__ llpre,
                                                     const float *__restrict__ suffix, const float *__restrict__ xend,
                                                     const float *__restrict__ rstart, float *__restrict__ ckpt,
                                                     double *__restrict__ loglik, const float *__restrict__ gw,
                                                     float *__restrict__ dE, float *__restrict__ gpart, long long wtot,
                                                     long long slot_base, int *__restrict__ wtab,
                                                     const int *__restrict__ wlist, int *__restrict__ wcnt,
                                                     int *__restrict__ flags, double *__restrict__ dfix, Plan p, float eps,
                                                     int ext0) {
    __shared__ __attribute__((aligned(16))) float ostage[4 * OUT_SEG];
    __shared__ __attribute__((aligned(16))) float tpose[4 * 2 * GR_TILE];
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    GradWindows pol;
    pol.gw = gw; pol.dE = dE; pol.gpart = gpart; pol.tps = tpose + w * (2 * GR_TILE);
    pol.wtot = wtot; pol.slot_base = slot_base; pol.b = p.b;
    window_walk(pol, A, E, prefix, llpre, suffix, xend, rstart, ckpt, loglik, wtab, wlist, wcnt, flags, dfix, p, eps, ext0,
                ostage + w * OUT_SEG);
}

// dA: fixed-order fp64 sum of the per-wave partials.  Stage 1: (model, slice) blocks; stage 2: one
// block per model.  256 threads = the 16x16 entries.
__global__ __launch_bounds__(256) void k_grad_sum1(const float *__restrict__ gpart, double *__restrict__ gred,
                                                   long long wpm) {
    const int m = blockIdx.y, sl = blockIdx.x;
    const long long w0 = wpm * sl / GR_SLICES, w1 = wpm * (sl + 1) / GR_SLICES;
    const float *src = gpart + ((size_t)m * wpm) * (QP * QP) + threadIdx.x;
    double acc = 0.0;
    for (long long w = w0; w < w1; ++w) acc += (double)src[(size_t)w * (QP * QP)];
    gred[((size_t)m * GR_SLICES + sl) * (QP * QP) + threadIdx.x] = acc;
}

__global__ __launch_bounds__(256) void k_grad_sum2(const double *__restrict__ gred, float *__restrict__ dA, int q) {
    const int m = blockIdx.x;
    double acc = 0.0;
    for (int sl = 0; sl < GR_SLICES; ++sl) acc += gred[((size_t)m * GR_SLICES + sl) * (QP * QP) + threadIdx.x];
    const int i = threadIdx.x / QP, j = threadIdx.x % QP;
    if (i < q && j < q) dA[((size_t)m * q + i) * q + j] = (float)acc;
}

// dpi[j] = sum_b gamma_0[j] w / pi[j], read back from the first row of dE (= w gamma_0 / max(E_0, eps), in clamped
// entries too: those are zeroed here, clamped emissions get no gradient).
__global__ __launch_bounds__(64) void k_grad_pi(const float *__restrict__ pi, const float *__restrict__ E,
                                                float *__restrict__ dE, int b, int L, int q, float eps,
                                                float *__restrict__ dpi) {
    // one wave per (model, state): lane s takes sequences s, s + 64, ..., fixed butterfly over the 64 partials
    const int m = blockIdx.y, j = blockIdx.x;
    double acc = 0.0;
    for (int s = threadIdx.x; s < b; s += 64) {
        const size_t o = ((size_t)m * b + s) * (size_t)L * q + j;
        const float e = E[o];
        acc += (double)dE[o] * (double)fmaxf(e, eps);
        if (!(e > eps)) dE[o] = 0.f;
    }
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if (threadIdx.x == 0) {
        const float pj = pi[(size_t)m * q + j];
        dpi[(size_t)m * q + j] = pj > eps ? (float)(acc / (double)pj) : 0.f;
    }
}

struct GradPlan {
    Plan p, px;                    // scan plan and serial exact-clamp plan
    long long wpm, wpmx;           // apply waves per model of either; wpm + wpmx + b gpart slots per model (b: one per
                                   // sequence for its windows)
    size_t o_gpart, o_gred, o_wckpt, total;   // o_wckpt: the windows' own checkpoint rows [seq][chunk][block] (the scan
                                              // plan's are read once more after the windows have run)
};

static int make_gradplan(int k, int b, int L, int q, GradPlan *gp) {
    int rc = make_plan(HMM_OP_POSTERIOR, k, b, L, q, &gp->p);
    if (rc) return rc;
    if ((rc = make_xplan(gp->p, &gp->px))) return rc;
    gp->wpm = apply_waves(gp->p) / k;
    gp->wpmx = apply_waves(gp->px) / k;
    size_t off = gp->p.total;
    gp->o_gpart = off; off = align_up(off + (size_t)k * (gp->wpm + gp->wpmx + b) * QP * QP * sizeof(float));
    gp->o_gred = off;  off = align_up(off + (size_t)k * GR_SLICES * QP * QP * sizeof(double));
    gp->o_wckpt = off; off = align_up(off + (size_t)gp->p.nchains * gp->p.nsub * QP * sizeof(float));
    gp->total = off;
    return HMM_OK;
}

// the compiled 29-state topology per chunk (hmm_postgrad_chunked.inc, defined after this file)
static bool pc_llgrad_wanted(int k, int b, int L, int q);
static size_t pc_llgrad_workspace(int k, int b, int L, int q);
static int pc_loglik_grad(const float *A, const float *pi, const float *E, int k, int b, int L, int q, float eps,
                          const float *gw, float *dA, float *dpi, float *dE, double *loglik, char *ws, size_t ws_bytes,
                          hipStream_t st);
static long long pc_llgrad_serial_count(int k, int b, int L, int q, const void *ws, size_t ws_bytes);

extern "C" {

int hmm_grad_max_states(void) { return MQ_MAX; }

size_t hmm_loglik_grad_workspace_bytes(int k, int b, int L, int q) {
    if (q > QP && q <= MQ_MAX) {
        if (k < 1 || b < 1 || L < 1) return 0;
        if (pc_llgrad_wanted(k, b, L, q)) return pc_llgrad_workspace(k, b, L, q);
        MqGradPlan mp;
        make_mqgradplan(k, b, q, &mp);
        return mp.total;
    }
    GradPlan gp;
    if (make_gradplan(k, b, L, q, &gp)) return 0;
    return gp.total;
}

long long hmm_loglik_grad_serial_count(int k, int b, int L, int q, const void *workspace, size_t workspace_bytes) {
    if (k < 1 || b < 1 || L < 1 || q < 1 || q > MQ_MAX) return HMM_ERR_BAD_SHAPE;
    if (q <= QP) {
        // read through the plan hmm_loglik_grad itself used (not the posterior's batch groups)
        GradPlan gp;
        int rc = make_gradplan(k, b, L, q, &gp);
        if (rc) return rc;
        if (!workspace) return HMM_ERR_NULL_POINTER;
        if (workspace_bytes < gp.total) return HMM_ERR_WORKSPACE;
        int v = 0;
        if (hipMemcpy(&v, Ws16(gp.p, workspace).nexact, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess)
            return HMM_ERR_LAUNCH;
        return v;
    }
    if (!pc_llgrad_wanted(k, b, L, q)) return (long long)k * b;
    return pc_llgrad_serial_count(k, b, L, q, workspace, workspace_bytes);
}

int hmm_loglik_grad(const float *A, const float *pi, const float *E, int k, int b, int L, int q, float eps,
                    const float *grad_loglik, float *dA, float *dpi, float *dE, double *loglik,
                    void *workspace, size_t workspace_bytes, void *stream) {
    if (q > QP && q <= MQ_MAX) {                             // one wave per sequence (hmm_midq.inc)
        if (k < 1 || b < 1 || L < 1) return HMM_ERR_BAD_SHAPE;
        if (!A || !pi || !E || !dA || !dpi || !dE || !workspace) return HMM_ERR_NULL_POINTER;
        if (check_eps(eps)) return HMM_ERR_BAD_ARGUMENT;
        if (pc_llgrad_wanted(k, b, L, q))
            return pc_loglik_grad(A, pi, E, k, b, L, q, eps, grad_loglik, dA, dpi, dE, loglik, (char *)workspace,
                                  workspace_bytes, (hipStream_t)stream);
        MqGradPlan mp;
        make_mqgradplan(k, b, q, &mp);
        if (workspace_bytes < mp.total || ((uintptr_t)workspace & 255)) return HMM_ERR_WORKSPACE;
        return mq_loglik_grad(A, pi, E, k, b, L, q, eps, grad_loglik, dA, dpi, dE, loglik, (char *)workspace,
                              (hipStream_t)stream);
    }
    GradPlan gp;
    int rc = make_gradplan(k, b, L, q, &gp);
    if (rc) return rc;
    if (!A || !pi || !E || !dA || !dpi || !dE || !workspace) return HMM_ERR_NULL_POINTER;
    if ((rc = check_eps(eps))) return rc;
    if (workspace_bytes < gp.total || ((uintptr_t)workspace & 255)) return HMM_ERR_WORKSPACE;
    const Plan &p = gp.p, &px = gp.px;
    char *ws = (char *)workspace;
    hipStream_t st = (hipStream_t)stream;
    if ((rc = run_reduce_scan(A, pi, E, p, eps, ws, st))) return rc;
    const Ws16 w(p, ws);
    const long long nw = apply_waves(p), nwx = apply_waves(px);
    const Routing rt = routing(w), rtf = routing_flagged(rt, w);
    float *gpart = ws_at<float>(ws, gp.o_gpart);
    double *gred = ws_at<double>(ws, gp.o_gred);
    const long long wtot = gp.wpm + gp.wpmx + b;
    launch(k_forward<true, false, false>, apply_grid(p), dim3(256), 0, st, A, pi, E, w.prefix, w.llpre, w.ckpt, nullptr,
           w.loglik, w.xend, rt, p, eps, nw, nullptr, nullptr);
    // the sequences' window slots of gpart: written only for sequences that have windows
    for (int m = 0; m < k; ++m)
        if (hipMemsetAsync(gpart + ((size_t)m * wtot + gp.wpm + gp.wpmx) * QP * QP, 0, (size_t)b * QP * QP * sizeof(float), st) !=
            hipSuccess)
            return HMM_ERR_LAUNCH;
    launch(k_backward_grad<false>, apply_grid(p), dim3(256), 0, st, A, E, w.ckpt, w.suffix, grad_loglik, dE, gpart, rt,
           gp.wpm, 0ll, wtot, p, eps, nw, w.phi, nullptr, nullptr, w.rstart);
    // the verdict per sequence; the flagged runs of chunks in windows; the scan plan's waves that hold routed chains
    // once more without them; the serial plan for sequences routed whole
    s16_select(p, w, rt, st);
    launch(k_window_grad, win_grid(p), dim3(256), 0, st, A, E, w.prefix, w.llpre, w.suffix, w.xend, w.rstart,
           ws_at<float>(ws, gp.o_wckpt), w.loglik, grad_loglik, dE, gpart, wtot, gp.wpm + gp.wpmx, w.wtab, w.wlist, w.wcnt,
           w.flags, w.dfix, p, eps, win_margin(p));
    launch(k_backward_grad<false>, apply_grid(p), dim3(256), 0, st, A, E, w.ckpt, w.suffix, grad_loglik, dE, gpart, rt,
           gp.wpm, 0ll, wtot, p, eps, nw, nullptr, w.flags, w.wtab, nullptr);
    launch(k_forward<true, false, true>, apply_grid(px), dim3(256), 0, st, A, pi, E, nullptr, nullptr, w.ckpt, nullptr,
           w.loglik, nullptr, rtf, px, eps, nwx, nullptr, nullptr);
    launch(k_backward_grad<true>, apply_grid(px), dim3(256), 0, st, A, E, w.ckpt, nullptr, grad_loglik, dE, gpart, rtf,
           gp.wpmx, gp.wpm, wtot, px, eps, nwx, nullptr, nullptr, nullptr, nullptr);
    launch(k_grad_sum1, dim3(GR_SLICES, k), dim3(256), 0, st, gpart, gred, wtot);
    launch(k_grad_sum2, dim3(k), dim3(256), 0, st, gred, dA, q);
    launch(k_grad_pi, dim3(q, k), dim3(64), 0, st, pi, E, dE, b, L, q, eps, dpi);
    if (loglik) launch(k_copy_loglik, dim3((p.NB + 255) / 256), dim3(256), 0, st, w.loglik, loglik, p.NB);
    return check_launch();
}

}  // extern "C"
