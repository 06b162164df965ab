// hmm_postgrad_chunked.inc — the sweeps of hmm_postgrad.inc cut into the chunks of the scan plan (q <= 16, and
// the compiled 29-state topology on hmm_scan_rows.inc's plan; included by hmm_postgrad.inc).  At the end of the
// file: the log-likelihood gradient of the 29-state topology on the same value sweeps.
//
// hmm_postgrad.inc walks four dependent chains over the whole sequence: 12 ms at the reference's own
// training shape (b = 32, L = 9 999, tests/parallel_rnn_forward.py:19-23) whatever the batch, one wave per
// sequence with 15 of its 64 lanes busy.  Per chunk the chains are independent once the vector ENTERING the
// chunk is known, and four chunks share a wave (a 16-lane row each; 32 states: two rows of 32):
//
//   values    alpha_hat entering a chunk is the chunk scan's prefix vector, Rb at a chunk's last position is
//             its suffix vector up to scale (run_reduce_scan) — the two value sweeps run one wave per
//             (sequence, chunk) with the step code of the serial sweeps, each warmed up over the neighbouring
//             chunk so that the floor-level components are the exact recursion's too (k_pc_values);
//   adjoints  both adjoint recursions are AFFINE in the adjoint vector: a chunk maps the vector entering it
//             to the vector leaving it as  out = J in + c.
//             c comes from running the chunk's sweep from a zero vector (k_pc_src).
//             J is the transposed Jacobian of the chunk's value map, which is the chunk operator W the reduce
//             kernel already left (W = B_t0 ... B_{t1-1}, B_t = A diag(E'_t)), normalised:
//                 alpha_hat_{t1-1} = alpha_hat_{t0-1} W / Z,   Z  = prod S_t          (t0 <= t < t1)
//                 Rb_{t0-1}        = W Rb_{t1-1} / Zb,         Zb = prod Sb_t
//             so, with a = d loss / d alpha_hat_{t1-1} and r = d loss / d Rb_{t0-1} the entering vectors,
//                 d loss / d alpha_hat_{t0-1} = W (a - <a, alpha_hat_{t1-1}>) / Z
//                 d loss / d Rb_{t1-1}        = W^T (r - <r, Rb_{t0-1}> / sum Rb_{t0-1}) / Zb
//             (the centring terms are the derivatives of the normalisers; both vanish in exact arithmetic,
//             because the loss is homogeneous of degree 0 in either vector, and are kept because they stop
//             rounding errors of the dominant state's component from travelling on).  The boundaries of the
//             backward recursion's adjoint therefore sit at the chunks' LAST positions.  k_pc_scan walks the
//             chunks of a sequence with these maps (one wave per sequence and direction, a W x W mat-vec
//             per hop) and leaves the vector entering every chunk; k_pc_final reruns the sweeps from those and
//             stores dE and the chunks' parts of dA and dpi.
//             (Measuring J by running the sweep on unit vectors instead — the first version — loses the
//             result to cancellation as soon as an emission of the dominant state is ~1e-10: the columns
//             are then 1e10 apart and meet again in the combination.)
//
// Same step arithmetic and fixed summation orders as the serial path inside the chunks: deterministic.
// The chunk operators carry the eps floors as ordinary (additive) weights and know nothing of the clamps'
// "pass nothing" rule; that is immaterial exactly when floor transitions are:
//
// Routing.  k_pc_src sums what decides that, and k_pc_scan flags the sequences the serial sweeps have to
// redo (`need`, all on the device, same call):
//   - models k_topo_check routed to the serial exact-clamp kernels (TOPO_EXACT; 32-state rows: k32_check);
//   - sequences over the engine's own certificate, F = eps * sum_t 1 / Sg_t > EXACT_DELTA (F bounds the
//     posterior probability that any floor transition is used);
//   - log mode: d loss / d log gamma_t[j] weighs the paths THROUGH (t, j), of which floor paths may be up to
//     F / gamma_t[j] however small F is.  With w = |G_t[j]| the weight that is exposed to the floors is at most
//     sum w min(1, F / gamma) <= F * sum_{gamma >= 1e-8} w / gamma + sum_{gamma < 1e-8} w;  flagged when that
//     exceeds PC_LOG_EXPOSED of sum w.

struct PcPlan {
    int W;                                   // states per row: 16 (main pipeline's scan plan), 32 or 64 (hmm_scan_mid.inc's)
    Plan p;                                  // shape and chunks
    MidPlan mid;                             // W = 32, 64: the scan plan of that width (its p is copied into `p`)
    PgPlan pg;                               // AH, RB, dEa, S, per-sequence partials (shared with the serial sweeps)
    size_t o_ops, o_exps, o_prefix, o_suffix, o_route;       // inside the scan plan's part of the workspace
    size_t o_pg, o_c, o_lam, o_gpart, o_side, o_need, o_sp, total;
};
#define PC_LOG_EXPOSED 1e-4f

// Chunk length of this path.  Its serial parts are the boundary scan (L / T hops of ~1.2 us) and the four
// sweeps a row walks one after the other (4 T steps of ~0.45 us): L / T * 1.2 + 1.8 T is smallest at
// T = sqrt(0.67 L) — 80 for L = 1e4, 256 for L = 1e5 (measured, tools/experiments/postgrad_chunk.py: b = 32 x
// 9 999 0.61 ms at the scan plan's 32, 0.47 at 64; two sequences of 1e5 1.80 at 64, 1.19 at 128) — and never
// shorter than the scan plan's own choice, which already sees enough parallelism at that length.
static int pc_chunk_len(int k, int b, int L) {
    const int t = choose_T((long long)k * b, L);
    if (opt(HMM_OPT_CHUNK) == t) return t;                   // set explicitly
    int ts = 16;
    while ((long long)ts * ts * 3 < 2ll * L && ts < MAX_T) ts += 16;
    const int lmax = ((L + 15) / 16) * 16;
    ts = ts > lmax ? lmax : ts;
    return t > ts ? t : ts;
}

// rows of 16 lanes for q <= 16; rows of 32 for the compiled 29-state topology (other 17..32-state models would
// all be handed back to the whole-sequence sweeps by k32_check)
static int pc_width(int q) { return q <= QP ? QP : (q == TopoGene29::Q ? Q32 : 0); }

// HMM_OPT_PGCHUNK: 0 never, 1 when it pays (few sequences, several chunks), 2 whenever the shape allows and
// for every sequence (no certificate; tests)
static bool pc_wanted(int k, int b, int L, int q) {
    const int o = opt(HMM_OPT_PGCHUNK);
    const int W = pc_width(q);
    if (o == 0 || W == 0) return false;
    if (q == 1) return false;                                // hmm_posterior_grad returns exact zeros: nothing to cut into chunks
    if ((long long)L * q * (long long)sizeof(float) >= (1ll << 31) - 4096) return false;   // 32-bit row offsets
    if ((long long)k * b > (1ll << 30) / 64) return false;
    const int T = pc_chunk_len(k, b, L), C = (L + T - 1) / T;
    if (C < 2) return false;
    if (o == 2) return true;
    // the whole-sequence sweeps cost the same for one sequence or a thousand (a wave each, ~1.2 us per
    // position); the chunked ones do twice the work, four chunks to the wave, at ~0.65 ns per (sequence,
    // position; b = 1024 x L = 1e5: 54 ms against 169, b = 2048 x 1e4: 13.5 against 24.5): ahead until the
    // whole-sequence waves would fill the machine several times over.  32-state rows: two chunks to the wave
    // and four times the arithmetic per step.
    return (long long)k * b <= (W == QP ? 4096 : 512) && C >= 4;
}

// W: the row width; 0 = pc_width's (hmm_grad_scan.inc and hmm_postgrad_scan.inc ask for Q32 / Q64 for any model of 17..64 states)
static int make_pcplan(int k, int b, int L, int q, PcPlan *pc, int W = 0) {
    if (W == 0) W = pc_width(q);
    if (W == 0) return HMM_ERR_Q_UNSUPPORTED;
    pc->W = W;
    size_t off;
    if (W == QP) {
        int rc = make_plan(HMM_OP_BACKWARD, k, b, L, q, &pc->p, pc_chunk_len(k, b, L));
        if (rc) return rc;
        pc->o_ops = pc->p.o_ops; pc->o_exps = pc->p.o_exps; pc->o_prefix = pc->p.o_prefix; pc->o_suffix = pc->p.o_suffix;
        pc->o_route = pc->p.o_topo;
        off = pc->p.total;
    } else {
        int rc = make_midplan(HMM_OP_BACKWARD, k, b, L, q, W, &pc->mid, pc_chunk_len(k, b, L));
        if (rc) return rc;
        pc->p = pc->mid.p;
        pc->o_ops = pc->mid.o_ops; pc->o_exps = pc->mid.o_exps; pc->o_prefix = pc->mid.o_prefix;
        pc->o_suffix = pc->mid.o_suffix; pc->o_route = pc->mid.o_elig;
        off = pc->mid.total;
    }
    make_pgplan(k, b, L, q, &pc->pg);
    const Plan &p = pc->p;
    pc->o_pg = off;    off = align_up(off + pc->pg.total);
    pc->o_c = off;     off = align_up(off + 2 * (size_t)p.nchains * W * sizeof(float));               // [dir][chain][W]
    pc->o_lam = off;   off = align_up(off + 2 * (size_t)p.nchains * W * sizeof(float));               // [dir][chain][W]
    pc->o_gpart = off; off = align_up(off + 2 * (size_t)p.nchains * q * q * sizeof(float));           // [dir][chain][q][q]
    pc->o_side = off;  off = align_up(off + 2 * (size_t)p.nchains * sizeof(PgSide));                  // [dir][chain]
    pc->o_need = off;  off = align_up(off + (size_t)p.NB * sizeof(int));
    pc->o_sp = off;    off = align_up(off + (size_t)k * sizeof(MqSp));             // sparse-step tables of the whole-sequence redo
    pc->total = off;
    return HMM_OK;
}

// ---- The sweeps of a chunk, SEVERAL chunks per wave: a chunk owns one row of W lanes (lane & (W-1) = state;
// W = 16: four chunks per wave, W = 32: two), sums are DPP (+ one permlane) reductions inside the row and a
// state's value reaches its row through the DPP row broadcast (W = 32: a readlane per half and a select) —
// the step code of hmm_postgrad.inc's whole-sequence sweeps (a wave per sequence, 15 of 64 lanes busy) at up
// to four times the work per instruction.  The rows of a wave walk different chunks (of different lengths at
// a sequence's end, possibly of different sequences and models), so the loops run to the longest row's count
// and every row carries its own `on` flag; a row that is done, or has nothing to do, keeps computing on
// harmless constants (no 0 * inf) and stores nothing.
template <int W> struct PcW;
template <> struct PcW<16> {
    static __device__ __forceinline__ float sum(float v) { return row_sum_f(v); }
    template <int K> static __device__ __forceinline__ float bc(float v) {      // lane K of this lane's row
        return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x150 + K, 0xF, 0xF, false));
    }
    // acc += (lane K of v's row) * c in ONE instruction: the row broadcast as the DPP modifier of the fma's first
    // operand (the compiler keeps v_mov_b32_dpp + v_fma apart).  Inline asm, so the "VALU write -> DPP read"
    // hazard of v is covered by hand: the first of a run of these waits two cycles.
    template <int K> static __device__ __forceinline__ void fmac_bc(float &acc, float v, float c) {
        if (K == 0)
            asm volatile("s_nop 1\n\tv_fmac_f32_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(v), "v"(c), "n"(K));
        else
            asm volatile("v_fmac_f32_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(v), "v"(c), "n"(K));
    }
    // which models the whole-sequence sweeps serve: k_topo_check's verdict
    static __device__ __forceinline__ bool model_serial(const int *route, int m) { return route[m] == TOPO_EXACT; }
};
template <> struct PcW<32> {
    static __device__ __forceinline__ float sum(float v) {                     // over the 32 lanes of this lane's half
        float a = row_sum_f(v), b = a;
        swap16(a, b);
        return a + b;
    }
    template <int K> static __device__ __forceinline__ float bc(float v) {
        const float lo = lane_bcast(v, K), hi = lane_bcast(v, 32 + K);
        return (threadIdx.x & 32) ? hi : lo;
    }
    template <int K> static __device__ __forceinline__ void fmac_bc(float &acc, float v, float c) { acc = fmaf(bc<K>(v), c, acc); }
    // k32_check's verdict (elig[m] = 0: not the compiled topology, or not primitive)
    static __device__ __forceinline__ bool model_serial(const int *route, int m) { return route[m] == 0; }
};
// one chunk per wave, lane = state: the row sum is the wave sum, and a state's value reaches the row as a readlane,
// which the fma takes as its scalar operand
template <> struct PcW<64> {
    static __device__ __forceinline__ float sum(float v) { return mq_wave_sum(v); }
    template <int K> static __device__ __forceinline__ float bc(float v) { return lane_bcast(v, K); }
    template <int K> static __device__ __forceinline__ void fmac_bc(float &acc, float v, float c) { acc = fmaf(bc<K>(v), c, acc); }
    // k64_check's verdict (elig[m] = Rows<4>::ID_DENSE, or 0: not primitive)
    static __device__ __forceinline__ bool model_serial(const int *route, int m) { return route[m] == 0; }
};
template <int W, int K> struct PcLoop {
    // r[K & 3] += v[K] * coef[K]  |  grow[K] += a * b[K]   for K .. W-1
    static __device__ __forceinline__ void matvec(float v, const float (&coef)[W], float (&r)[4]) {
        PcW<W>::template fmac_bc<K>(r[K & 3], v, coef[K]);
        PcLoop<W, K + 1>::matvec(v, coef, r);
    }
    static __device__ __forceinline__ void outer(float a, float b, float (&grow)[W]) {
        PcW<W>::template fmac_bc<K>(grow[K], b, a);
        PcLoop<W, K + 1>::outer(a, b, grow);
    }
};
template <int W> struct PcLoop<W, W> {
    static __device__ __forceinline__ void matvec(float, const float (&)[W], float (&)[4]) {}
    static __device__ __forceinline__ void outer(float, float, float (&)[W]) {}
};
// sum_k v[k] * coef[k] over the states of the row (coef: this lane's W coefficients)
template <int W>
__device__ __forceinline__ float pc_row_matvec(float v, const float (&coef)[W]) {
    float r[4] = {0.f, 0.f, 0.f, 0.f};
    PcLoop<W, 0>::matvec(v, coef, r);
    return (r[0] + r[1]) + (r[2] + r[3]);
}
// grow[k] += a * (lane k of b's row)
template <int W>
__device__ __forceinline__ void pc_row_outer(float a, float b, float (&grow)[W]) { PcLoop<W, 0>::outer(a, b, grow); }
__device__ __forceinline__ int pc_wave_max_i(int v) {
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
    return v;
}

// what a row works on
struct PcRow {
    long long chain;
    int seq, c, m, x;
    bool valid, act;             // the row has a chunk of a model this path serves; and this lane a state of it
    size_t base;                 // element offset of the sequence in the (k,b,L,q) tensors
};
template <int W>
__device__ __forceinline__ PcRow pc_row(const Plan &p, const int *route) {
    PcRow r;
    const int lane = threadIdx.x & 63;
    r.chain = (long long)blockIdx.x * (64 / W) + lane / W;
    r.x = lane & (W - 1);
    r.valid = r.chain < p.nchains;
    const long long ch = r.valid ? r.chain : 0;
    r.seq = (int)(ch / p.C);
    r.c = (int)(ch - (long long)r.seq * p.C);
    r.m = r.seq / p.b;
    r.valid = r.valid && !PcW<W>::model_serial(route, r.m);
    r.act = r.valid && r.x < p.q;
    r.base = (size_t)r.seq * p.L * p.q;
    return r;
}

// the local adjoint of pg_local (hmm_postgrad.inc) with row sums
template <int W>
__device__ __forceinline__ void pc_local(float G, float al, float rb, bool act, int mode, float *ga, float *gr,
                                         float *inv_sg, float *gamma) {
    const float g = act ? al * rb : 0.f;
    const float ig = __builtin_amdgcn_rcpf(PcW<W>::sum(g));
    *inv_sg = ig;
    *gamma = g * ig;
    if (mode == 0) {
        const float dot = PcW<W>::sum(act ? G * g * ig : 0.f);
        const float gb = act ? (G - dot) * ig : 0.f;
        *ga = gb * al;
        *gr = gb * rb;
    } else {
        const float c = PcW<W>::sum(act ? G : 0.f) * ig;
        *ga = act ? (rb > 0.f ? G / rb : 0.f) - c * al : 0.f;
        *gr = act ? (al > 0.f ? G / al : 0.f) - c * rb : 0.f;
    }
}

// ---- value sweeps.  blockIdx.y = 0: alpha_hat (sign bit = the clamp of the predicted state was active) and
// the normalisers S_t; 1: Rb (sign bit = clamp active).
// Each sweep WARMS UP over the neighbouring chunk: it starts from the scan's vector one chunk further away and
// stores only its own positions.  The scan's vectors are right in every component that carries weight, but
// their floor-level components (states the clamp holds at eps) come from additive floors; a floor-level
// component is re-made by the clamps within a step or two of the exact recursion, so after a chunk of it the
// vector entering the stored positions is the exact recursion's in all components, and so are the clamp bits.
// (Components that are small but above eps are not re-made, they travel — along the codon cycles of the gene
// models for hundreds of positions — and keep the scan's relative error eps / component; PC_WARMUP steps at
// least, whatever the chunk length, keep that below what the adjoint of an ABSENT edge can see.)
#define PC_WARMUP 64
template <int W>
__global__ __launch_bounds__(64) void k_pc_values(const float *__restrict__ A, const float *__restrict__ E,
                                                  const float *__restrict__ prefix, const float *__restrict__ suffix,
                                                  const int *__restrict__ topo, Plan p, float eps,
                                                  float *__restrict__ AH, float *__restrict__ S,
                                                  float *__restrict__ RB) {
    const PcRow r = pc_row<W>(p, topo);
    const int q = p.q, L = p.L, x = r.x;
    const bool act = r.act;
    const int t0 = r.c * p.T, t1 = min(L, t0 + p.T);
    const float *Am = A + (size_t)r.m * q * q;
    const size_t base = r.base;
    auto ldE = [&](int t) { return (act && t >= 0 && t < L) ? E[base + (size_t)t * q + x] : 0.f; };
    const float uni = x < q ? 1.f / (float)q : 0.f;          // what a row that is done computes on
    if (blockIdx.y == 0) {
        float acol[W];
#pragma unroll
        for (int i = 0; i < W; ++i) acol[i] = (act && i < q) ? Am[(size_t)i * q + x] : 0.f;
        // from the chunk before (with short chunks: as many as make PC_WARMUP steps): its prefix vector is
        // alpha_hat of the position before IT (chunk 0: the start distribution as it is)
        const int cs = max(r.c - (PC_WARMUP + p.T - 1) / p.T, 0), ts = cs * p.T;
        float v = act ? prefix[((size_t)r.seq * p.C + cs) * W + x] : uni;
        if (cs > 0 || !r.valid) v *= __builtin_amdgcn_rcpf(PcW<W>::sum(v));
        const int nmax = pc_wave_max_i(r.valid ? t1 - ts : 0);
        float en = ldE(ts);
        for (int n = 0; n < nmax; ++n) {
            const int t = ts + n;
            const bool on = r.valid && t < t1;
            const float e = on ? fmaxf(en, eps) : 1.f;
            en = ldE(t + 1);
            const float Rm = pc_row_matvec<W>(v, acol);
            const float R = (on && t > 0) ? Rm : v;
            const float sf = x < q ? e * fmaxf(R, eps) : 0.f;
            const float Ssum = PcW<W>::sum(sf);
            const float vn = sf * __builtin_amdgcn_rcpf(Ssum);
            v = on ? vn : uni;
            if (on && t >= t0) {
                if (x == 0) S[(size_t)r.seq * L + t] = Ssum;
                if (act) AH[base + (size_t)t * q + x] = !(R > eps) ? -vn : vn;
            }
        }
    } else {
        float arow[W];
#pragma unroll
        for (int j = 0; j < W; ++j) arow[j] = (act && j < q) ? Am[(size_t)x * q + j] : 0.f;
        // from the last position of the chunk after: ones at the end of the sequence, otherwise that chunk's
        // suffix vector, whose scale is arbitrary (bh is scale-free: everything after the first step is not)
        const int ce = min(r.c + (PC_WARMUP + p.T - 1) / p.T, p.C - 1), te = min(L, (ce + 1) * p.T);
        float rb = act ? suffix[((size_t)r.seq * p.C + ce) * W + x] : uni;
        if (te == L) rb = x < q ? 1.f : 0.f;
        if (t1 == L && act) RB[base + (size_t)(L - 1) * q + x] = 1.f;
        // steps t = te-1 .. t0+1: bh_t from Rb_t, then Rb_{t-1}
        const int nmax = pc_wave_max_i(r.valid ? te - 1 - t0 : 0);
        float en = ldE(te - 1);
        for (int n = 0; n < nmax; ++n) {
            const int t = te - 1 - n;
            const bool on = r.valid && t > t0;
            const float e = on ? fmaxf(en, eps) : 1.f;
            en = ldE(t - 1);
            const float sb = x < q ? e * rb : 0.f;
            const float bh = sb * __builtin_amdgcn_rcpf(PcW<W>::sum(sb));
            const float raw = pc_row_matvec<W>(bh, arow);
            const float rn = fmaxf(raw, eps);
            if (on && act && t - 1 < t1) RB[base + (size_t)(t - 1) * q + x] = raw > eps ? rn : -rn;
            rb = on ? rn : uni;
        }
    }
}

// The steps of chunk c: the adjoint of the forward recursion covers the chunk's own positions; the adjoint of the
// backward recursion the steps t -> t+1 from the last position of the chunk before to the chunk's own last
// position (the last chunk: to the end of the sequence) — see the head of the file.
__device__ __forceinline__ void pc_range(const Plan &p, int c, int dir, int *t0, int *t1) {
    const int a = c * p.T, b = min(p.L, a + p.T);
    if (dir == 0) { *t0 = max(a - 1, 0); *t1 = c == p.C - 1 ? p.L : b - 1; }
    else { *t0 = a; *t1 = b; }
}

// ---- the adjoint sweeps of pg_beta_body / pg_alpha_body (hmm_postgrad.inc), row-packed.  on a row:
//   dir 0  Rbar_in = d loss / d Rb_{t0} -> d loss / d Rb_{t1}, steps t -> t+1 for t in [t0, t1), t + 1 < L
//   dir 1  abar_in = d loss / d alpha_hat_{t1-1} (from the future) -> d loss / d alpha_hat_{t0-1}, positions t1-1 .. t0
// ACC: store dE and the chunk's part of dA (row x of it in lane x) and of dpi.  Returns the leaving vector;
// sd: the routing sums and the product of the normalisers (valid in every lane of the row).
template <int W, bool ACC, class GL = PgStateG>
__device__ __forceinline__ float pc_beta_sweep(const PcRow &r, const float *__restrict__ A, const float *__restrict__ E,
                                               const float *__restrict__ AH, const float *__restrict__ RB,
                                               const GL G, const Plan &p, float eps, int mode, int t0,
                                               int t1, float Rbar_in, PgSide *sd, float *__restrict__ dEb,
                                               float *__restrict__ gp) {
    const int q = p.q, L = p.L, x = r.x;
    const bool act = r.act;
    const float *Am = A + (size_t)r.m * q * q;
    float acol[W], grow[W];
#pragma unroll
    for (int i = 0; i < W; ++i) { acol[i] = (act && i < q) ? Am[(size_t)i * q + x] : 0.f; grow[i] = 0.f; }
    const size_t base = r.base;
    auto ld = [&](const float *ptr, int t) { return (act && t < L) ? ptr[base + (size_t)t * q + x] : 0.f; };
    const float *Gx = G.seq((size_t)r.seq, L, q) + G.col(x);          // the loader (hmm_postgrad.inc): this state's column
    const int gq = G.stride(q);
    auto ldG = [&](int t) { return (act && t < L) ? Gx[(size_t)t * gq] : 0.f; };
    const float uni = x < q ? 1.f / (float)q : 0.f;
    float rbs = ld(RB, t0);
    float Rbar = Rbar_in;
    if (__builtin_amdgcn_ballot_w64(r.valid && t0 == 0) != 0ull) {    // R-bar of position 0: only the output term
        const bool first = r.valid && t0 == 0;
        float ga, gr, isg, gam;
        pc_local<W>(first ? ldG(0) : 0.f, first ? __builtin_fabsf(ld(AH, 0)) : uni, first ? __builtin_fabsf(rbs) : 1.f,
                 x < q, mode, &ga, &gr, &isg, &gam);
        if (first) Rbar = ga;
        if (ACC && first && act) dEb[base + x] = 0.f;         // bh_0 feeds nothing
    }
    const int nmax = pc_wave_max_i(r.valid ? min(t1, L - 1) - t0 : 0);
    float e1n = ld(E, t0 + 1), rb1n = ld(RB, t0 + 1), al1n = ld(AH, t0 + 1), g1n = ldG(t0 + 1);
    float zm = 1.f;
    int ze = 0;
    for (int n = 0; n < nmax; ++n) {
        const int t = t0 + n;
        const bool on = r.valid && t < t1 && t + 1 < L;
        const float e1 = on ? fmaxf(e1n, eps) : 1.f, rb1s = on ? rb1n : 1.f, al1 = on ? __builtin_fabsf(al1n) : uni;
        const float G1 = on ? g1n : 0.f;
        e1n = ld(E, t + 2); rb1n = ld(RB, t + 2); al1n = ld(AH, t + 2); g1n = ldG(t + 2);
        const float rb1 = __builtin_fabsf(rb1s);
        const float w = (on && act && __builtin_bit_cast(int, rbs) >= 0) ? Rbar : 0.f;     // clamp of Rb_t passes nothing
        const float sb = x < q ? e1 * rb1 : 0.f;
        const float Sb = PcW<W>::sum(sb);
        const float iSb = __builtin_amdgcn_rcpf(Sb);
        if (on) {
            zm *= Sb;
            ze += __builtin_amdgcn_frexp_expf(zm);
            zm = __builtin_amdgcn_frexp_mantf(zm);
        }
        const float bh1 = sb * iSb;
        if (ACC) pc_row_outer<W>(w, bh1, grow);                  // dA[x][i] += w[x] bh_{t+1}[i]
        const float bhbar = pc_row_matvec<W>(w, acol);           // bhbar[x] = sum_i A[i][x] w[i]
        const float dot = PcW<W>::sum(x < q ? bhbar * bh1 : 0.f);
        const float vbar = x < q ? (bhbar - dot) * iSb : 0.f;
        if (ACC && on && act) dEb[base + (size_t)(t + 1) * q + x] = vbar * rb1;
        float ga, gr, isg, gam;
        pc_local<W>(G1, al1, rb1, x < q, mode, &ga, &gr, &isg, &gam);
        Rbar = on ? ga + vbar * e1 : Rbar;
        rbs = on ? rb1s : rbs;
    }
    sd->zman = zm; sd->zexp = ze;
    if (ACC && act) {
#pragma unroll
        for (int i = 0; i < W; ++i)
            if (i < q) gp[i] = grow[i];
    }
    return act ? Rbar : 0.f;
}

template <int W, bool ACC, class GL = PgStateG>
__device__ __forceinline__ float pc_alpha_sweep(const PcRow &r, const float *__restrict__ A, const float *__restrict__ pi,
                                                const float *__restrict__ E, const float *__restrict__ AH,
                                                const float *__restrict__ Sst, const float *__restrict__ RB,
                                                const GL G, const Plan &p, float eps, int mode, int t0,
                                                int t1, float abar_in, PgSide *sd, float *__restrict__ dEa,
                                                float *__restrict__ gp, float *__restrict__ dpi_part) {
    const int q = p.q, L = p.L, x = r.x;
    const bool act = r.act;
    const float *Am = A + (size_t)r.m * q * q;
    float arow[W], grow[W];
#pragma unroll
    for (int j = 0; j < W; ++j) { arow[j] = (act && j < q) ? Am[(size_t)x * q + j] : 0.f; grow[j] = 0.f; }
    const size_t base = r.base;
    auto ld = [&](const float *ptr, int t) { return (act && t >= 0) ? ptr[base + (size_t)t * q + x] : 0.f; };
    const float *Gx = G.seq((size_t)r.seq, L, q) + G.col(x);          // the loader (hmm_postgrad.inc): this state's column
    const int gq = G.stride(q);
    auto ldG = [&](int t) { return (act && t >= 0) ? Gx[(size_t)t * gq] : 0.f; };
    auto ldS = [&](int t) { return (r.valid && t >= 0) ? Sst[(size_t)r.seq * L + t] : 1.f; };
    const float uni = x < q ? 1.f / (float)q : 0.f;
    float abar = abar_in;                                    // d loss / d alpha_t from the future
    const int nmax = pc_wave_max_i(r.valid ? t1 - t0 : 0);
    float en = ld(E, t1 - 1), ahn = ld(AH, t1 - 1), rbn = ld(RB, t1 - 1), gn = ldG(t1 - 1), Sn = ldS(t1 - 1);
    float phis = 0.f, c_p = 0.f, c_q = 0.f, c_t = 0.f, zm = 1.f;
    int ze = 0;
    for (int n = 0; n < nmax; ++n) {
        const int t = t1 - 1 - n;
        const bool on = r.valid && t >= t0;
        const float e = on ? fmaxf(en, eps) : 1.f, ahs = on ? ahn : uni, rb = on ? __builtin_fabsf(rbn) : 1.f;
        const float Gt = on ? gn : 0.f, Sv = on ? Sn : 1.f;
        en = ld(E, t - 1); ahn = ld(AH, t - 1); rbn = ld(RB, t - 1); gn = ldG(t - 1); Sn = ldS(t - 1);
        const float al = __builtin_fabsf(ahs);
        float ga, gr, isg, gam;
        pc_local<W>(Gt, al, rb, x < q, mode, &ga, &gr, &isg, &gam);
        if (on) {
            zm *= Sv;
            ze += __builtin_amdgcn_frexp_expf(zm);
            zm = __builtin_amdgcn_frexp_mantf(zm);
            phis += isg;
            const float wg = act ? __builtin_fabsf(Gt) : 0.f;
            const bool tiny = !(gam >= PG_TINY_GAMMA);
            c_t += wg;
            c_q += tiny ? wg : 0.f;
            c_p += tiny ? 0.f : wg * __builtin_amdgcn_rcpf(gam);
        }
        const float ab = abar + gr;
        const float dot = PcW<W>::sum(x < q ? ab * al : 0.f);
        const float ubar = x < q ? (ab - dot) * __builtin_amdgcn_rcpf(Sv) : 0.f;
        const float Rf = al * Sv * __builtin_amdgcn_rcpf(e);                          // max(R^f_t, eps) = u_t / E'_t
        if (ACC && on && act) dEa[base + (size_t)t * q + x] = ubar * Rf;
        const float Rfbar = (on && act && __builtin_bit_cast(int, ahs) >= 0) ? ubar * e : 0.f;   // clamp of R^f_t passes nothing
        const float alp = (on && t > 0) ? __builtin_fabsf(ahn) : 0.f;                // alpha_hat_{t-1}[x]
        if (ACC) pc_row_outer<W>(alp, Rfbar, grow);                                       // dA[x][j] += alpha_{t-1}[x] Rfbar[j]
        const float nb = pc_row_matvec<W>(Rfbar, arow);                                   // abar_{t-1}[x] = sum_j A[x][j] Rfbar[j]
        if (ACC && on && act && t == 0) dpi_part[(size_t)r.seq * q + x] = pi[(size_t)r.m * q + x] > eps ? Rfbar : 0.f;
        abar = on ? (t > 0 ? nb : 0.f) : abar;
    }
    sd->inv_sg = phis;
    sd->g_over_gamma = PcW<W>::sum(c_p);
    sd->g_tiny = PcW<W>::sum(c_q);
    sd->g_all = PcW<W>::sum(c_t);
    sd->zman = zm; sd->zexp = ze;
    if (ACC && act) {
#pragma unroll
        for (int j = 0; j < W; ++j)
            if (j < q) gp[j] = grow[j];
    }
    return act ? abar : 0.f;
}

// ---- the inhomogeneous part of every chunk's map: the adjoint sweeps from a zero vector, nothing stored
// but the vector leaving the chunk, the routing sums and the products of the normalisers.
// blockIdx.y: 0 = adjoint of the backward recursion (ascending), 1 = of the forward recursion (descending)
template <int W, class GL = PgStateG>
__global__ __launch_bounds__(64) void k_pc_src(const float *__restrict__ A, const float *__restrict__ pi,
                                               const float *__restrict__ E, const float *__restrict__ AH,
                                               const float *__restrict__ Sst, const float *__restrict__ RB,
                                               const GL G, const int *__restrict__ topo, Plan p,
                                               float eps, int mode, float *__restrict__ cvec, PgSide *__restrict__ sides) {
    const PcRow r = pc_row<W>(p, topo);
    const int dir = blockIdx.y;
    int t0, t1;
    pc_range(p, r.c, dir, &t0, &t1);
    PgSide sd = {0.f, 0.f, 0.f, 0.f, 1.f, 0};
    const float out = dir == 0 ? pc_beta_sweep<W, false>(r, A, E, AH, RB, G, p, eps, mode, t0, t1, 0.f, &sd, nullptr, nullptr)
                               : pc_alpha_sweep<W, false>(r, A, pi, E, AH, Sst, RB, G, p, eps, mode, t0, t1, 0.f, &sd, nullptr,
                                                       nullptr, nullptr);
    if (!r.valid) return;
    cvec[((size_t)dir * p.nchains + r.chain) * W + r.x] = out;
    if (r.x == 0) sides[(size_t)dir * p.nchains + r.chain] = sd;
}

// ---- the vectors entering every chunk: one wave per (sequence, direction) walks the sequence's chunks;
// the wave of direction 0 also decides which sequences the serial sweeps have to redo
__device__ __forceinline__ float pc_scale(float v, int e) {          // v * 2^e, e of any size
    e = e < -250 ? -250 : (e > 250 ? 250 : e);
    const int h = e / 2;
    return __builtin_amdgcn_ldexpf(__builtin_amdgcn_ldexpf(v, h), e - h);
}

#define PCS_PF 1        // hops of loads in flight (4 changed nothing: 0.6 us per hop is the dependent arithmetic)
template <int W>
__global__ __launch_bounds__(64) void k_pc_scan(const float *__restrict__ ops, const int *__restrict__ exps,
                                                const float *__restrict__ AH, const float *__restrict__ RB,
                                                const float *__restrict__ cvec, const PgSide *__restrict__ sides,
                                                const int *__restrict__ topo, Plan p, float eps, int mode,
                                                int exact_mode, int force, float *__restrict__ lam,
                                                int *__restrict__ need, const int *__restrict__ risk = nullptr) {
    const int seq = blockIdx.x, dir = blockIdx.y, x = threadIdx.x & 63, n = x & (W - 1);
    const int C = p.C, q = p.q, L = p.L;
    const size_t ch0 = (size_t)seq * C;
    const bool model_exact = PcW<W>::model_serial(topo, seq / p.b);
    if (dir == 0) {
        float s = 0.f, gp = 0.f, gq = 0.f, gt = 0.f;
        bool mark = false;                                   // risk (or null): the reduces' marks, as k_pc_llselect reads them
        if (!model_exact) {
            const int el = topo[seq / p.b];
            for (int c = x; c < C; c += 64) {
                const PgSide sd = sides[(size_t)p.nchains + ch0 + c];               // (the sums are the descending sweep's)
                s += sd.inv_sg; gp += sd.g_over_gamma; gq += sd.g_tiny; gt += sd.g_all;
                if (risk) mark = mark || (elig_dense(el) ? risk[ch0 + c] != 0 : exps[(ch0 + c) * W + W - 1] != 0);
            }
        }
        mark = __builtin_amdgcn_ballot_w64(mark) != 0ull;
        const float F = mq_wave_sum(s) * eps;
        gp = mq_wave_sum(gp); gq = mq_wave_sum(gq); gt = mq_wave_sum(gt);
        bool flagged = !(F <= EXACT_DELTA);                                           // (also catches inf / NaN)
        if (mode == HMM_POST_LOG) flagged = flagged || !(F * gp + gq <= PC_LOG_EXPOSED * gt);
        flagged = (flagged || mark) && !force && exact_mode == HMM_EXACT_AUTO;
        if (x == 0) need[seq] = (model_exact || flagged) ? 1 : 0;
    }
    if (model_exact) return;
    const size_t base = (size_t)seq * L * q;
    const float *cv = cvec + ((size_t)dir * p.nchains + ch0) * W;
    const PgSide *sd = sides + (size_t)dir * p.nchains + ch0;
    float *lm = lam + ((size_t)dir * p.nchains + ch0) * W;
    // what a hop through chunk c needs — the operator (dir 0: row n; dir 1: column n), the exponent of this lane's
    // source state, the value vector of the centring term, the normaliser, the chunk's own part — is loaded
    // PCS_PF hops ahead into a ring of slots
    float w[PCS_PF][W];
    int xe[PCS_PF], ze[PCS_PF];
    float val[PCS_PF], zm[PCS_PF], cn[PCS_PF];
    auto fetch = [&](int u, int c) {
        const float *X = ops + (ch0 + c) * W * W;
        if (dir == 0) {
#pragma unroll
            for (int k = 0; k < W; k += 4) {
                const f4 r = *reinterpret_cast<const f4 *>(X + n * W + k);
                w[u][k] = r.x; w[u][k + 1] = r.y; w[u][k + 2] = r.z; w[u][k + 3] = r.w;
            }
        } else {
#pragma unroll
            for (int k = 0; k < W; ++k) w[u][k] = X[k * W + n];
        }
        xe[u] = exps[(ch0 + c) * W + n];
        const int tv = dir == 0 ? c * p.T - 1 : min(L, (c + 1) * p.T) - 1;         // Rb_{t0-1} | alpha_hat_{t1-1}
        val[u] = n < q ? __builtin_fabsf((dir == 0 ? RB : AH)[base + (size_t)tv * q + n]) : 0.f;
        zm[u] = sd[c].zman; ze[u] = sd[c].zexp;
        cn[u] = cv[(size_t)c * W + n];                       // the chunk's own (inhomogeneous) part
    };
#pragma unroll
    for (int u = 0; u < PCS_PF; ++u) {
        xe[u] = 0; ze[u] = 0; val[u] = 0.f; zm[u] = 1.f; cn[u] = 0.f;
#pragma unroll
        for (int k = 0; k < W; ++k) w[u][k] = 0.f;
    }
    if (dir == 0) {
        // ascending: r_c = d loss / d Rb at the last position of chunk c - 1, entering chunk c
        float v = cv[n];                                      // leaves chunk 0 (nothing entered it)
        if (x < W) lm[x] = 0.f;
#pragma unroll
        for (int u = 0; u < PCS_PF; ++u)
            if (1 + u < C) fetch(u, 1 + u);
        for (int cb = 1; cb < C; cb += PCS_PF)
#pragma unroll
          for (int u = 0; u < PCS_PF; ++u) {
            const int c = cb + u;
            if (c >= C) break;                                // wave-uniform
            if (x < W) lm[(size_t)c * W + x] = v;
            float wc[W];
#pragma unroll
            for (int k = 0; k < W; ++k) wc[k] = w[u][k];
            const int xec = xe[u], zec = ze[u];
            const float valc = val[u], zmc = zm[u], cnc = cn[u];
            if (c + PCS_PF < C) fetch(u, c + PCS_PF);
            // centre, scale the source states (column k of W is 2^exps[k] times the stored one), apply W^T
            const float sc = PcW<W>::sum(v * valc) * __builtin_amdgcn_rcpf(PcW<W>::sum(valc));   // (every row holds the same W values)
            const float uu = n < q ? pc_scale((v - sc) * __builtin_amdgcn_rcpf(zmc), xec - zec) : 0.f;
            float o0 = 0.f, o1 = 0.f;
#pragma unroll
            for (int k = 0; k < W; k += 2) {
                o0 = fmaf(lane_bcast(uu, k), wc[k], o0);
                o1 = fmaf(lane_bcast(uu, k + 1), wc[k + 1], o1);
            }
            v = (n < q ? o0 + o1 : 0.f) + cnc;
        }
    } else {
        // descending: a_c = d loss / d alpha_hat at the last position of chunk c (from the future), entering chunk c
        float v = 0.f;
#pragma unroll
        for (int u = 0; u < PCS_PF; ++u)
            if (C - 1 - u >= 1) fetch(u, C - 1 - u);
        for (int cb = C - 1; cb >= 1; cb -= PCS_PF)
#pragma unroll
          for (int u = 0; u < PCS_PF; ++u) {
            const int c = cb - u;
            if (c < 1) break;                                 // wave-uniform
            if (x < W) lm[(size_t)c * W + x] = v;
            float wc[W];
#pragma unroll
            for (int k = 0; k < W; ++k) wc[k] = w[u][k];
            const int xec = xe[u], zec = ze[u];
            const float valc = val[u], zmc = zm[u], cnc = cn[u];
            if (c - PCS_PF >= 1) fetch(u, c - PCS_PF);
            const float sc = PcW<W>::sum(v * valc);                                      // (alpha_hat sums to 1)
            const float uu = n < q ? v - sc : 0.f;
            float o0 = 0.f, o1 = 0.f;
#pragma unroll
            for (int k = 0; k < W; k += 2) {
                o0 = fmaf(lane_bcast(uu, k), wc[k], o0);
                o1 = fmaf(lane_bcast(uu, k + 1), wc[k + 1], o1);
            }
            v = (n < q ? pc_scale((o0 + o1) * __builtin_amdgcn_rcpf(zmc), xec - zec) : 0.f) + cnc;
        }
        if (x < W) lm[x] = v;
    }
}

// ---- log mode of hmm_class_posterior_grad (hmm_class_posterior.inc): the adjoints run in prob mode on G' = Gc / P, so
// k_pc_scan's log rule is off, and the class analogue is applied here, between k_pc_scan and k_pc_final: a sequence
// is flagged when  F sum_{P_c >= 1e-8} |Gc| / P_c + sum_{P_c < 1e-8} |Gc|  >  PC_LOG_EXPOSED sum |Gc|.
// F is formed as k_pc_scan forms it (the same loads and sums in the same order); the three sums are the pre-pass's
// (k_cp_quot: `parts` fp64 triples per sequence, summed here in index order).  One wave per sequence.
template <int W>
__global__ __launch_bounds__(64) void k_pc_class_rule(const PgSide *__restrict__ sides, const int *__restrict__ topo, Plan p,
                                                      float eps, int exact_mode, int force,
                                                      const double *__restrict__ csum, int parts, int *__restrict__ need) {
    const int seq = blockIdx.x, x = threadIdx.x & 63;
    if (PcW<W>::model_serial(topo, seq / p.b) || force || exact_mode != HMM_EXACT_AUTO) return;
    const size_t ch0 = (size_t)seq * p.C;
    float s = 0.f;
    for (int c = x; c < p.C; c += 64) s += sides[(size_t)p.nchains + ch0 + c].inv_sg;
    const float F = mq_wave_sum(s) * eps;
    double gp = 0.0, gq = 0.0, gt = 0.0;
    for (int i = 0; i < parts; ++i) {
        const double *t = csum + ((size_t)seq * parts + i) * 3;
        gp += t[0]; gq += t[1]; gt += t[2];
    }
    if (x == 0 && !(F * (float)gp + (float)gq <= PC_LOG_EXPOSED * (float)gt)) need[seq] = 1;
}

// ---- the sweeps again, from the true entering vectors, storing dE and the chunks' parts of dA and dpi
template <int W, class GL = PgStateG>
__global__ __launch_bounds__(64) void k_pc_final(const float *__restrict__ A, const float *__restrict__ pi,
                                                 const float *__restrict__ E, const float *__restrict__ AH,
                                                 const float *__restrict__ Sst, const float *__restrict__ RB,
                                                 const GL G, const int *__restrict__ topo,
                                                 const int *__restrict__ need, Plan p, float eps, int mode,
                                                 const float *__restrict__ lam, float *__restrict__ dEb,
                                                 float *__restrict__ dEa, float *__restrict__ gpart,
                                                 float *__restrict__ dpi_part) {
    PcRow r = pc_row<W>(p, topo);
    if (r.valid && need[r.seq]) { r.valid = false; r.act = false; }      // the whole-sequence sweeps redo this sequence
    const int dir = blockIdx.y, q = p.q;
    int t0, t1;
    pc_range(p, r.c, dir, &t0, &t1);
    const long long ch = r.chain < p.nchains ? r.chain : 0;
    const float vin = r.act ? lam[((size_t)dir * p.nchains + ch) * W + r.x] : 0.f;
    float *gp = gpart + (((size_t)dir * p.nchains + ch) * q + r.x) * q;
    PgSide sd;
    if (dir == 0)
        pc_beta_sweep<W, true>(r, A, E, AH, RB, G, p, eps, mode, t0, t1, vin, &sd, dEb, gp);
    else
        pc_alpha_sweep<W, true>(r, A, pi, E, AH, Sst, RB, G, p, eps, mode, t0, t1, vin, &sd, dEa, gp, dpi_part);
}

// per-sequence parts of dA from the chunks' (fp64, fixed order), in the serial sweeps' layout: one wave per
// (entry, sequence, direction), lane c takes chunks c, c + 64, ..., the 64 partials meet in a fixed butterfly
// (one thread per entry walking all the chunks: 28 us of the 0.46 ms call at b = 32 x L = 9 999)
__global__ __launch_bounds__(64) void k_pc_fold(const float *__restrict__ gpart, const int *__restrict__ need, Plan p,
                                                float *__restrict__ gb, float *__restrict__ ga) {
    const int e = blockIdx.x, seq = blockIdx.y, dir = blockIdx.z, qq = p.q * p.q;
    if (need[seq]) return;
    const float *src = gpart + ((size_t)dir * p.nchains + (size_t)seq * p.C) * qq + e;
    double acc = 0.0;
    for (int c = threadIdx.x; c < p.C; c += 64) acc += (double)src[(size_t)c * qq];
    acc = pg_wave_sum_d(acc);
    if (threadIdx.x == 0) (dir == 0 ? gb : ga)[(size_t)seq * qq + e] = (float)acc;
}

// the same with one block per (sequence, direction), a thread per entry walking the chunks: for batches that fill
// the machine with blocks anyway (the wave-per-entry grid is 2 q^2 blocks per sequence)
__global__ __launch_bounds__(256) void k_pc_fold_seq(const float *__restrict__ gpart, const int *__restrict__ need,
                                                     Plan p, int ndir, float *__restrict__ gb, float *__restrict__ ga) {
    const int seq = blockIdx.x, dir = blockIdx.y, qq = p.q * p.q;
    if (need[seq]) return;
    for (int e = threadIdx.x; e < qq; e += 256) {
        const float *src = gpart + ((size_t)dir * p.nchains + (size_t)seq * p.C) * qq + e;
        double acc = 0.0;
        for (int c = 0; c < p.C; ++c) acc += (double)src[(size_t)c * qq];
        (dir == 0 ? gb : ga)[(size_t)seq * qq + e] = (float)acc;
    }
}
#define PC_FOLD_WAVES_MAX_SEQS 256        // up to here a wave per entry, above a block per sequence

// risk (or null): the dense reduces' per-chain marks flag a sequence as well (hmm_postgrad_scan.inc; hmm_posterior_grad's
// own paths run without)
// csum (or null): the class log rule's sums, `cparts` triples per sequence (k_pc_class_rule)
template <int W, class GL>
static int pc_launch_w(const float *A, const float *pi, const float *E, int k, int b, int L, int q, float eps, int mode,
                       const GL G, float *dA, float *dpi, float *dE, char *ws, const PcPlan &pc, hipStream_t st,
                       const int *risk = nullptr, const double *csum = nullptr, int cparts = 0) {
    const Plan &p = pc.p;
    const PgPlan &pp = pc.pg;
    char *wp = ws + pc.o_pg;
    float *AH = (float *)(wp + pp.o_ah), *RB = (float *)(wp + pp.o_rb), *S = (float *)(wp + pp.o_s);
    float *dEa = (float *)(wp + pp.o_dea);
    float *gb = (float *)(wp + pp.o_gpart), *ga = (float *)(wp + pp.o_gpart2), *dpp = (float *)(wp + pp.o_dpi);
    float *cvec = (float *)(ws + pc.o_c), *lam = (float *)(ws + pc.o_lam), *gpart = (float *)(ws + pc.o_gpart);
    PgSide *sides = (PgSide *)(ws + pc.o_side);
    int *need = (int *)(ws + pc.o_need);
    const int *route = (const int *)(ws + pc.o_route);
    const dim3 chains2((unsigned)((p.nchains + 64 / W - 1) / (64 / W)), 2);       // 64 / W chunks per wave
    hipLaunchKernelGGL(k_pc_values<W>, chains2, dim3(64), 0, st, A, E, (const float *)(ws + pc.o_prefix),
                       (const float *)(ws + pc.o_suffix), route, p, eps, AH, S, RB);
    hipLaunchKernelGGL((k_pc_src<W, GL>), chains2, dim3(64), 0, st, A, pi, E, (const float *)AH, (const float *)S,
                       (const float *)RB, G, route, p, eps, mode, cvec, sides);
    hipLaunchKernelGGL(k_pc_scan<W>, dim3(p.NB, 2), dim3(64), 0, st, (const float *)(ws + pc.o_ops),
                       (const int *)(ws + pc.o_exps), (const float *)AH, (const float *)RB, (const float *)cvec,
                       (const PgSide *)sides, route, p, eps, mode, opt(HMM_OPT_EXACT), opt(HMM_OPT_PGCHUNK) == 2 ? 1 : 0,
                       lam, need, risk);
    if (csum)
        hipLaunchKernelGGL(k_pc_class_rule<W>, dim3(p.NB), dim3(64), 0, st, (const PgSide *)sides, route, p, eps,
                           opt(HMM_OPT_EXACT), opt(HMM_OPT_PGCHUNK) == 2 ? 1 : 0, csum, cparts, need);
    hipLaunchKernelGGL((k_pc_final<W, GL>), chains2, dim3(64), 0, st, A, pi, E, (const float *)AH, (const float *)S,
                       (const float *)RB, G, route, (const int *)need, p, eps, mode, (const float *)lam, dE, dEa, gpart, dpp);
    if (p.NB <= PC_FOLD_WAVES_MAX_SEQS)
        hipLaunchKernelGGL(k_pc_fold, dim3(q * q, p.NB, 2), dim3(64), 0, st, (const float *)gpart, (const int *)need, p, gb, ga);
    else
        hipLaunchKernelGGL(k_pc_fold_seq, dim3(p.NB, 2), dim3(256), 0, st, (const float *)gpart, (const int *)need, p, 2, gb, ga);
    // the serial sweeps for what is flagged (their waves exit at once otherwise), then the common tail.  The redo is
    // hmm_posterior_grad's own instantiation for q, bit for bit: rows of 64 serve 33..48 states with k_pg_*<48>
    if constexpr (W == Q64) {
        if (q <= 48) pg_launch<48>(A, pi, E, k, b, L, q, eps, mode, G, dA, dE, wp, pp, st, need);
        else pg_launch<W>(A, pi, E, k, b, L, q, eps, mode, G, dA, dE, wp, pp, st, need);
    } else {
        pg_launch<W>(A, pi, E, k, b, L, q, eps, mode, G, dA, dE, wp, pp, st, need);
    }
    hipLaunchKernelGGL(k_pg_sum_rows, dim3(q, k), dim3(64), 0, st, (const float *)dpp, dpi, b, q);
    return check_launch();
}

static int pc_launch(const float *A, const float *pi, const float *E, int k, int b, int L, int q, float eps, int mode,
                     const PgStateG G, float *dA, float *dpi, float *dE, char *ws, const PcPlan &pc, hipStream_t st) {
    if (pc.W == QP) {
        int rc = run_reduce_scan(A, pi, E, pc.p, eps, ws, st);
        if (rc) return rc;
        return pc_launch_w<QP>(A, pi, E, k, b, L, q, eps, mode, G, dA, dpi, dE, ws, pc, st);
    }
    scan_reduce_scan<Scan32>(A, pi, E, pc.mid, eps, ws, st);
    return pc_launch_w<Q32>(A, pi, E, k, b, L, q, eps, mode, G, dA, dpi, dE, ws, pc, st);
}

// ------------------------------------------------------------------ log-likelihood gradients per chunk
// hmm_loglik_grad for the compiled 29-state topology (17..64 states otherwise: two whole-sequence sweeps,
// hmm_midq.inc; q <= 16: the MFMA kernels of hmm_grad.inc).  dE = w gamma / E, dA = sum_t xi_t / A and dpi need
// no adjoint recursion at all: with alpha_hat and Rb of every position in place (k_pc_values) each chunk
// sums its own positions and transitions, and the log-likelihood is the scan's.  Routing as above (model:
// k32_check; sequence: the floor-transition certificate); flagged sequences are redone by the whole-sequence
// sweeps with a mask.
template <int W>
__global__ __launch_bounds__(64) void k_pc_llgrad(const float *__restrict__ A, const float *__restrict__ E,
                                                  const float *__restrict__ AH, const float *__restrict__ RB,
                                                  const float *__restrict__ gw, const int *__restrict__ route, Plan p,
                                                  float eps, float *__restrict__ dE, float *__restrict__ gpart,
                                                  float *__restrict__ inv_sg) {
    const PcRow r = pc_row<W>(p, route);
    const int q = p.q, L = p.L, x = r.x;
    const bool act = r.act;
    const int t0 = r.c * p.T, t1 = min(L, t0 + p.T);
    const size_t base = r.base;
    auto ld = [&](const float *ptr, int t) { return (act && t < L) ? ptr[base + (size_t)t * q + x] : 0.f; };
    const float uni = x < q ? 1.f / (float)q : 0.f;
    const float w = r.valid ? (gw ? gw[r.seq] : 1.f) : 0.f;
    float grow[W];
#pragma unroll
    for (int j = 0; j < W; ++j) grow[j] = 0.f;
    const int nmax = pc_wave_max_i(r.valid ? t1 - t0 : 0);
    float en = ld(E, t0), an = ld(AH, t0), rn = ld(RB, t0);
    float phis = 0.f;
    for (int n = 0; n < nmax; ++n) {
        const int t = t0 + n;
        const bool on = r.valid && t < t1, has = on && t + 1 < L;
        const float eraw = en, e = on ? fmaxf(eraw, eps) : 1.f;
        const float al = on ? __builtin_fabsf(an) : uni, rb = on ? __builtin_fabsf(rn) : 1.f;
        en = ld(E, t + 1); an = ld(AH, t + 1); rn = ld(RB, t + 1);          // position t + 1: this step's transition, next step's own
        const float g = x < q ? al * rb : 0.f;
        const float ig = __builtin_amdgcn_rcpf(PcW<W>::sum(g));
        if (on) phis += ig;
        // (position 0 keeps w gamma_0 / eps in its clamped entries for k_mq_grad_pi, which zeroes them)
        if (on && act) dE[base + (size_t)t * q + x] = (eraw > eps || t == 0) ? g * (ig * w) * __builtin_amdgcn_rcpf(e) : 0.f;
        // transition (t -> t + 1): row x of sum xi / A; nothing flows through a clamped predicted state of t + 1
        const float e1 = has ? fmaxf(en, eps) : 1.f, rb1 = has ? __builtin_fabsf(rn) : 1.f;
        const float sb = x < q ? e1 * rb1 : 0.f;
        const float bh = sb * __builtin_amdgcn_rcpf(PcW<W>::sum(sb));
        const float bhm = (has && act && __builtin_bit_cast(int, an) >= 0) ? bh : 0.f;
        pc_row_outer<W>((has && act) ? al * (ig * w) : 0.f, bhm, grow);
    }
    if (!r.valid) return;
    if (act) {
        float *gp = gpart + ((size_t)r.chain * q + x) * q;
#pragma unroll
        for (int j = 0; j < W; ++j)
            if (j < q) gp[j] = grow[j];
    }
    if (x == 0) inv_sg[r.chain] = phis;
}

// need[seq]: the whole-sequence sweeps redo it.  One wave per sequence.  exps / risk (or null): the reduces' marks
// as k_scan_select reads them — a chain whose operator went through the denormal range, or survives an observation at
// the emission floor only, flags its sequence.
template <int W>
__global__ __launch_bounds__(64) void k_pc_llselect(const float *__restrict__ inv_sg, const int *__restrict__ route, Plan p,
                                                    float eps, int exact_mode, int force, int *__restrict__ need,
                                                    const int *__restrict__ exps = nullptr,
                                                    const int *__restrict__ risk = nullptr) {
    const int seq = blockIdx.x;
    const int el = route[seq / p.b];
    const bool model_serial = PcW<W>::model_serial(route, seq / p.b);
    float s = 0.f;
    bool mark = false;
    if (!model_serial)
        for (int c = threadIdx.x; c < p.C; c += 64) {
            const size_t chain = (size_t)seq * p.C + c;
            s += inv_sg[chain];
            if (risk) mark = mark || (elig_dense(el) ? risk[chain] != 0 : exps[chain * W + W - 1] != 0);
        }
    const float F = mq_wave_sum(s) * eps;
    mark = __builtin_amdgcn_ballot_w64(mark) != 0ull;
    const bool flagged = (!(F <= EXACT_DELTA) || mark) && !force && exact_mode == HMM_EXACT_AUTO;
    if (threadIdx.x == 0) need[seq] = (model_serial || flagged) ? 1 : 0;
}

// the chunks' parts of dA folded into the per-sequence partial (fp64, fixed order): one wave per (entry, sequence)
__global__ __launch_bounds__(64) void k_pc_llfold(const float *__restrict__ gpart, const int *__restrict__ need, Plan p,
                                                  float *__restrict__ gseq) {
    const int e = blockIdx.x, seq = blockIdx.y, qq = p.q * p.q;
    if (need[seq]) return;
    const float *src = gpart + (size_t)seq * p.C * qq + e;
    double acc = 0.0;
    for (int c = threadIdx.x; c < p.C; c += 64) acc += (double)src[(size_t)c * qq];
    acc = pg_wave_sum_d(acc);
    if (threadIdx.x == 0) gseq[(size_t)seq * qq + e] = (float)acc;
}

static bool pc_llgrad_wanted(int k, int b, int L, int q) { return pc_width(q) == Q32 && pc_wanted(k, b, L, q); }
static size_t pc_llgrad_workspace(int k, int b, int L, int q) {
    PcPlan pc;
    return make_pcplan(k, b, L, q, &pc) ? 0 : pc.total;
}
// S: Scan32 / Scan64 (hmm_scan_mid.inc), or a type with their interface; pc: make_pcplan's for S::W.  marks: the
// reduces' risk marks flag a sequence as well (hmm_grad_scan.inc; the 29-state path of hmm_loglik_grad runs without).
template <class S>
static int pc_loglik_grad_on(const float *A, const float *pi, const float *E, int k, int b, int L, int q, float eps,
                             const float *gw, float *dA, float *dpi, float *dE, double *loglik, char *ws, const PcPlan &pc,
                             bool marks, hipStream_t st) {
    constexpr int W = S::W;
    const Plan &p = pc.p;
    const PgPlan &pp = pc.pg;
    scan_reduce_scan<S>(A, pi, E, pc.mid, eps, ws, st);
    char *wp = ws + pc.o_pg;
    float *AH = (float *)(wp + pp.o_ah), *RB = (float *)(wp + pp.o_rb), *S_ = (float *)(wp + pp.o_s);
    float *gseq = (float *)(wp + pp.o_gpart), *gpart = (float *)(ws + pc.o_gpart), *inv_sg = (float *)(ws + pc.o_c);
    double *ll = (double *)(ws + pc.mid.o_loglik);
    int *need = (int *)(ws + pc.o_need);
    const int *route = (const int *)(ws + pc.o_route);
    const unsigned nb = (unsigned)((p.nchains + 64 / W - 1) / (64 / W));
    hipLaunchKernelGGL(k_pc_values<W>, dim3(nb, 2), dim3(64), 0, st, A, E, (const float *)(ws + pc.o_prefix),
                       (const float *)(ws + pc.o_suffix), route, p, eps, AH, S_, RB);
    hipLaunchKernelGGL(k_pc_llgrad<W>, dim3(nb), dim3(64), 0, st, A, E, (const float *)AH, (const float *)RB, gw, route,
                       p, eps, dE, gpart, inv_sg);
    hipLaunchKernelGGL(k_pc_llselect<W>, dim3(p.NB), dim3(64), 0, st, (const float *)inv_sg, route, p, eps,
                       opt(HMM_OPT_EXACT), opt(HMM_OPT_PGCHUNK) == 2 ? 1 : 0, need,
                       marks ? (const int *)(ws + pc.o_exps) : nullptr, marks ? (const int *)(ws + pc.mid.o_risk) : nullptr);
    if (p.NB <= PC_FOLD_WAVES_MAX_SEQS)
        hipLaunchKernelGGL(k_pc_llfold, dim3(q * q, p.NB), dim3(64), 0, st, (const float *)gpart, (const int *)need, p, gseq);
    else
        hipLaunchKernelGGL(k_pc_fold_seq, dim3(p.NB, 1), dim3(256), 0, st, (const float *)gpart, (const int *)need, p, 1, gseq,
                           gseq);
    // the whole-sequence sweeps for what is flagged (their waves exit at once otherwise), then the sums
    return mq_loglik_grad_run(A, pi, E, k, b, L, q, eps, gw, dA, dpi, dE, loglik, ll, gseq, st, need, (MqSp *)(ws + pc.o_sp));
}
static int pc_loglik_grad(const float *A, const float *pi, const float *E, int k, int b, int L, int q, float eps,
                          const float *gw, float *dA, float *dpi, float *dE, double *loglik, char *ws, size_t ws_bytes,
                          hipStream_t st) {
    PcPlan pc;
    int rc = make_pcplan(k, b, L, q, &pc);
    if (rc) return rc;
    if (ws_bytes < pc.total || ((uintptr_t)ws & 255)) return HMM_ERR_WORKSPACE;
    return pc_loglik_grad_on<Scan32>(A, pi, E, k, b, L, q, eps, gw, dA, dpi, dE, loglik, ws, pc, false, st);
}
// W: make_pcplan's
static long long pc_llgrad_serial_count_w(int k, int b, int L, int q, const void *ws, size_t ws_bytes, int W) {
    PcPlan pc;
    int rc = make_pcplan(k, b, L, q, &pc, W);
    if (rc) return rc;
    if (!ws) return HMM_ERR_NULL_POINTER;
    if (ws_bytes < pc.total) return HMM_ERR_WORKSPACE;
    std::vector<int> need((size_t)pc.p.NB);
    if (hipMemcpy(need.data(), (const char *)ws + pc.o_need, need.size() * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess)
        return HMM_ERR_LAUNCH;
    long long n = 0;
    for (int v : need) n += v != 0;
    return n;
}
static long long pc_llgrad_serial_count(int k, int b, int L, int q, const void *ws, size_t ws_bytes) {
    return pc_llgrad_serial_count_w(k, b, L, q, ws, ws_bytes, 0);
}
