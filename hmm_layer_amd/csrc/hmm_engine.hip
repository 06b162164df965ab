// hmm_engine.hip — MI355X (gfx950 / CDNA4) HMM forward / backward / posterior engine.
//
// The per-timestep recurrence of the reference (hmm_layer/MsaHmmCell.py:73-106, driven by
// the Python loop hmm_layer/BaseRNN.py:217-227) is restructured as a three-phase scan
// over time chunks whose combine is a states x states matrix product on the f32 MFMA
// (v_mfma_f32_16x16x4_f32, exact f32 fma chain):
//
//   reduce  one wave per (sequence, chunk): the chunk operator  X <- diag(E_t) A^T X
//           (16 conditional forward vectors = the columns of one 16x16 MFMA tile),
//           columns rescaled by exact powers of two with integer exponent carry.
//           This is the reference's parallel_factor mode (hmm_layer/MsaHmmCell.py:122-142)
//           in linear space; one operator serves both directions.
//   scan    one wave per sequence: chunk-level prefix (alpha_hat entering each chunk)
//           and suffix (beta leaving each chunk) vectors — the role of
//           TotalProbabilityCell (hmm_layer/TotalProbabilityCell.py:30-49).
//   apply   one wave per 16 (sequence, chunk) pairs (the 16 columns of the MFMA tile):
//           exact cell-step semantics from the true prefix / suffix; forward pass writes
//           alpha_hat checkpoints every 16 steps, backward pass recomputes alpha_hat per
//           16-step block in registers and emits posteriors.
//
// MFMA operand trick: D = Aop * X accumulates over k in 4 steps; lane (g = lane>>4,
// n = lane&15) supplies k = 4g + kk at step kk instead of the canonical g + 4kk.  The
// permutation is applied to both operands, so the product is unchanged, and the output
// layout (row 4g + r, col n in register r) IS the next step's B-operand layout: the
// recurrence chains through registers with no transposes and no LDS.
//
// Layouts: everything the caller passes is row-major fp32 (k,b,L,q), q <= 16.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <mutex>
#include <type_traits>
#include <vector>
#include "hmm_engine.h"

typedef float f4 __attribute__((ext_vector_type(4)));
typedef int i4 __attribute__((ext_vector_type(4)));

#ifndef HMM_REDUCE_PF
#define HMM_REDUCE_PF 8        // emission rows in flight ahead of the reduce recurrence
#endif
#ifndef HMM_NT_STORE
#define HMM_NT_STORE 1  // posteriors / log alpha / log beta / dE leave through non-temporal 16-byte stores
#endif
#ifndef HMM_PSI
#define HMM_PSI 1       // experiments only: 0 compiles the clamp-born-mass sums out of k_backward (nothing is routed then)
#endif
#ifndef HMM_BWD_FULL
#define HMM_BWD_FULL 0  // k_backward: waves whose chains all own a full chunk skip the per-lane step masks — A/B in one
                        // process: 3.27 ms with, 2.97 without (two copies of the unrolled block)
#endif
#ifndef HMM_FWD_PF2
#define HMM_FWD_PF2 0
#endif
#ifndef HMM_CK_LD_NT
#define HMM_CK_LD_NT 0
#endif
#ifndef HMM_LD_AUX
#define HMM_LD_AUX 0   // cache-policy bits of the apply kernels' emission loads (experiments: 2 = nt)
#endif
#define QP 16          // padded state count = MFMA tile edge (scan kernels: q <= 16)
#define HMM_LARGEQ_MAX 4096   // serial-in-time GEMM path for 16 < q <= this
#ifndef HMM_SUB
#define HMM_SUB 8      // steps per apply block = alpha_hat checkpoint spacing
#endif
#define SUB HMM_SUB
#ifndef HMM_COALESCE_F
#define HMM_COALESCE_F 1   // apply kernels load emission rows in the coalesced loader layout (see permute_rows)
#endif
#ifndef HMM_COALESCE_B
#define HMM_COALESCE_B 0
#endif
#ifndef HMM_STAGE_BF
#define HMM_STAGE_BF 1     // stage_row without exec-mask regions: a component past the row goes to the chain's pad slot
#endif
#ifndef HMM_COLSUM2
#define HMM_COLSUM2 1      // backward step: gamma's and beta's normalisers in one paired column sum (col_sum2)
#endif
// (A/B of the two, profiles/apply_diet_ab.txt: k_backward<0,.,.,16> 2.79-2.94 ms with neither, 2.69-2.83 with the staging,
//  2.81-2.93 with the paired sum alone, 2.63-2.77 with both; bit-identical outputs; with both 0 the code before them)
#ifndef SCAN_PF
#define SCAN_PF 1      // hops of operator loads in flight in the group-level scan kernels.  These kernels are
                       // bandwidth-bound, not latency-bound (k_scan_inner reads the 345 MB of chunk operators in 65 us):
                       // four hops in flight changed nothing in k_scan_inner and cost k_scan_compose 50 -> 73 us
#endif
#define SCAN2_MIN_C 32  // chunks per sequence from which the chunk-level scan runs in two levels
#define MAX_T 512      // longest chunk: the ceiling of choose_T.  Where choose_T stops at it and the apply kernels need more
                       // than one round of resident blocks, round_T picks the chunk of the <= 16-state plans below it
// What the round-aware chunk rule (round_T) takes the machine to hold, as constants so that a plan stays a pure function
// of the shape (hmm_chunk_len and hmm_workspace_bytes are called without a device); hmm_plan_capacity returns them and
// tests/test_chunk_rounds_gpu.py holds them against the occupancy query and the CU count of the device.
#define PLAN_CUS 256          // compute units of an MI355X
#define PLAN_APPLY_BPC 2      // resident 4-wave blocks per CU of k_forward<true,...,16> / k_backward<0,...,16> (LDS: 66 KB each)
#define PLAN_REDUCE_BPC 4     // ... of k_reduce_sparse<TopoGene15> (128 VGPRs, 34 KB of LDS)
#define LN2 0.69314718055994530942

// ---- tuning / test options.  Explicit process-wide settings (hmm_set_option); the HMM_ENGINE_*
// environment variables only seed them, once, the first time any option is read.  The defaults
// are the measured best; results never depend on anything else outside a call's arguments.
#include <atomic>
static std::atomic<int> g_opt[HMM_OPT_COUNT];
static std::once_flag g_opt_once;
static void opt_seed() {
    static const char *names[HMM_OPT_COUNT] = {"HMM_ENGINE_CHUNK", "HMM_ENGINE_FORCE_DENSE", "HMM_ENGINE_SCAN2",
                                               "HMM_ENGINE_GROUPS", "HMM_ENGINE_EXACT", "HMM_ENGINE_PGCHUNK",
                                               "HMM_ENGINE_VGROUPS", "HMM_ENGINE_VLARGE", "HMM_ENGINE_GLARGE"};
    static const int defaults[HMM_OPT_COUNT] = {0, 0, 1, 1, HMM_EXACT_AUTO, 1, 0, 0, 0};
    for (int i = 0; i < HMM_OPT_COUNT; ++i) {
        const char *v = getenv(names[i]);
        g_opt[i].store(v ? atoi(v) : defaults[i]);
    }
}
static int opt(int which) {
    std::call_once(g_opt_once, opt_seed);
    return g_opt[which].load(std::memory_order_relaxed);
}

struct Plan {
    int k, b, L, q;
    int NB;            // k*b sequences
    int T, C;          // chunk length (multiple of SUB), chunks per sequence
    int nsub;          // T / SUB
    long long nchains; // NB * C
    int cpw;           // (sequence, chunk) pairs per apply wave: 16 = the tile's columns (1: exact plan of a very long sequence)
    int seq_start;     // 1: position 0 of the tensor is the first observation of its sequence (no transition into it);
                       // 0: a later time slab of a sequence-sharded call (hmm_seqshard_*)
    // workspace offsets (bytes)
    int G, gsize;      // two-level chunk scan: G groups of gsize chunks per sequence (G = 0: single level)
    size_t o_ops, o_exps, o_prefix, o_llpre, o_suffix, o_lsuf, o_ckpt, o_loglik, o_topo, total;
    size_t o_phi, o_nexact;   // exact-clamp routing: per-chain certificate sums psi [nchains], counter of routed sequences
    size_t o_flags;           // ... and the per-sequence verdict k_exact_select derives from them (ROUTE_*)
    size_t o_xend, o_rstart;  // alpha_hat after / R before every chain, as the scan plan's apply kernels stepped them
    size_t o_wtab, o_wlist, o_wcnt, o_dfix;   // window table [seq][WIN_STRIDE], sequences with windows, counters, loglik shifts
    size_t o_wshift;                          // per window: its log-likelihood shift and last chunk [seq][WSH_STRIDE doubles] (log alpha)
    size_t o_upi;                             // a uniform start distribution (k,q) (hmm_backward's certificate)
    size_t o_gops, o_gexps, o_gprefix, o_gllpre, o_gsuffix, o_glsuf;
};

static size_t align_up(size_t x) { return (x + 255) & ~(size_t)255; }
#define PLAN_WIN_STRIDE 34    // = WIN_STRIDE (window table, see k_exact_select)
#define PLAN_WSH_STRIDE 24    // = WSH_STRIDE: WIN_MAX doubles (shifts) + WIN_MAX ints (last chunks)

static int choose_T(long long NB, int L) {
    {                                                        // tuning knob, multiple of 16
        const int t = opt(HMM_OPT_CHUNK);
        if (t >= 16 && t <= MAX_T && t % 16 == 0) return t;
    }
    // enough (sequence, chunk) pairs to fill 256 CUs x 4 SIMDs in the apply kernels (16 pairs per
    // wave, two waves per SIMD: 32 768 pairs), chunks no longer than MAX_T, at least 16.
    long long t = (NB * (long long)L) / 32768;
    // ... but with few sequences that rule shreds a long sequence into tens of thousands of chunks
    // while a chunk is still a serial walk for its wave.  With the two-level chunk scans the serial
    // parts of a pass are T in-chunk steps and ~3 sqrt(L / T) scan hops of about one step's latency
    // each: T + 3 sqrt(L / T) is smallest at T = (1.5 sqrt(L))^(2/3), i.e. T^3 = 2.25 L — never go below
    // that (L = 1e6: 144, L = 1e5: 64; measured optimum for one sequence of 1e6: 128-256, for two of 1e5: 64,
    // tools/experiments/long_seq_chunks.py).
    long long tb = 16;
    while (tb * tb * tb * 4 < 9ll * L && tb < MAX_T) tb += 16;
    if (t < tb) t = tb;
    t = ((t + 16 - 1) / 16) * 16;
    if (t < 16) t = 16;
    if (t > MAX_T) t = MAX_T;
    long long lmax = (((long long)L + 16 - 1) / 16) * 16;
    if (t > lmax) t = lmax;
    return (int)t;
}

// The apply kernels' blocks at chunk length T: 16 (sequence, chunk) pairs per wave, 4 waves per block (apply_grid).
static long long plan_apply_blocks(int k, int b, int L, int T) {
    const long long C = (L + T - 1) / T;
    return ((long long)k * (((long long)b * C + 15) / 16) + 3) / 4;
}
// Modelled cost of a pass at chunk length T, in units of 0.8 ns.  Measured (profiles/rounds_sweep.txt, every multiple of
// 16 from 256 to 512 at six shapes): k_forward and k_backward take T steps times the blocks the fullest CU serves,
// ceil(blocks / PLAN_CUS), at ~650 ns per step for the pair — a CU's two resident blocks share its rate, so the quantum
// is one block per CU, half a round of resident blocks; b = 1024 x L = 1e5: 13 x 512 at T = 512, 14 x 448 at 448.  Every
// chunk costs the reduce and the scans ~0.8 ns for its operator (1/800 of a step).  The sparse reduce itself shows no
// such steps in T (1.36 +- 0.01 ms from 12.25 to 23 rounds of its resident blocks), so it has no term here.
#define PLAN_STEP_W 800
static long long plan_cost(int k, int b, int L, int T) {
    const long long per_cu = (plan_apply_blocks(k, b, L, T) + PLAN_CUS - 1) / PLAN_CUS;
    return PLAN_STEP_W * per_cu * T + (long long)k * b * ((L + T - 1) / T);
}
// The chunk length of the <= 16-state plans.  choose_T's, except where that is MAX_T and the apply kernels need more
// than one round of resident blocks: there the cheapest multiple of 16 from MAX_T down to half of it, never below
// choose_T's T^3 = 2.25 L floor; ties go to the longer chunk.  Smaller problems have fewer blocks than the machine holds
// and choose_T has already sized their chunks for that.  HMM_OPT_CHUNK forces T as before.
static int round_T(int k, int b, int L) {
    const int t0 = choose_T((long long)k * b, L);
    const int forced = opt(HMM_OPT_CHUNK);
    if (forced >= 16 && forced <= MAX_T && forced % 16 == 0) return t0;
    // one round of resident blocks: 64 (sequence, chunk) pairs to the block (choose_T's 32 768 pairs)
    if (t0 != MAX_T || (long long)k * b * ((L + t0 - 1) / t0) <= 64ll * PLAN_CUS * PLAN_APPLY_BPC) return t0;
    int lo = 16;
    while ((long long)lo * lo * lo * 4 < 9ll * L && lo < MAX_T) lo += 16;
    if (lo < t0 / 2) lo = t0 / 2;
    int best = t0;
    for (int t = t0 - 16; t >= lo; t -= 16)
        if (plan_cost(k, b, L, t) < plan_cost(k, b, L, best)) best = t;
    return best;
}

static int make_plan(int op, int k, int b, int L, int q, Plan *p, int T_fixed = 0) {
    if (k < 1 || b < 1 || L < 1 || q < 1) return HMM_ERR_BAD_SHAPE;
    if (q > QP) return HMM_ERR_Q_UNSUPPORTED;
    if ((long long)k * b > (1ll << 30) / 64) return HMM_ERR_BAD_SHAPE;
    p->k = k; p->b = b; p->L = L; p->q = q;
    p->NB = k * b;
    p->T = T_fixed ? T_fixed : round_T(k, b, L);
    p->C = (L + p->T - 1) / p->T;
    p->nsub = p->T / SUB;
    p->nchains = (long long)p->NB * p->C;
    p->cpw = 16;
    p->seq_start = 1;
    size_t off = 0;
    p->o_ops = off;    off = align_up(off + (size_t)p->nchains * QP * QP * sizeof(float));
    p->o_exps = off;   off = align_up(off + (size_t)p->nchains * QP * sizeof(int));
    p->o_prefix = off; off = align_up(off + (size_t)p->nchains * QP * sizeof(float));
    p->o_llpre = off;  off = align_up(off + (size_t)p->nchains * sizeof(double));
    p->o_suffix = off; off = align_up(off + (size_t)p->nchains * QP * sizeof(float));
    p->o_lsuf = off;   off = align_up(off + (size_t)p->nchains * sizeof(double));
    p->o_loglik = off; off = align_up(off + (size_t)p->NB * sizeof(double));
    p->o_topo = off;   off = align_up(off + (size_t)p->k * sizeof(int));
    p->o_phi = off;    off = align_up(off + (size_t)p->nchains * sizeof(float));
    p->o_nexact = off; off = align_up(off + sizeof(int));
    p->o_flags = off;  off = align_up(off + (size_t)p->NB * sizeof(int));
    p->o_xend = off;   off = align_up(off + (size_t)p->nchains * QP * sizeof(float));
    p->o_rstart = off; off = align_up(off + (size_t)p->nchains * QP * sizeof(float));
    p->o_wtab = off;   off = align_up(off + (size_t)p->NB * PLAN_WIN_STRIDE * sizeof(int));
    p->o_wlist = off;  off = align_up(off + (size_t)p->NB * sizeof(int));
    p->o_wcnt = off;   off = align_up(off + 4 * sizeof(int));
    p->o_dfix = off;   off = align_up(off + (size_t)p->NB * sizeof(double));
    p->o_wshift = off; off = align_up(off + ((op == HMM_OP_FORWARD || op == HMM_OP_BACKWARD) ? (size_t)p->NB * PLAN_WSH_STRIDE * sizeof(double) : 0));
    p->o_upi = off;    off = align_up(off + (size_t)p->k * p->q * sizeof(float));
    // two-level scan once the serial chain is long enough to matter (see k_scan_compose)
    p->G = 0; p->gsize = 0;
    if (p->C >= SCAN2_MIN_C) {
        int gs = 1;
        while (gs * gs < p->C) ++gs;
        p->gsize = gs;
        p->G = (p->C + gs - 1) / gs;
    }
    const size_t ng = (size_t)p->NB * (p->G > 0 ? p->G : 1);
    p->o_gops = off;    off = align_up(off + ng * QP * QP * sizeof(float));
    p->o_gexps = off;   off = align_up(off + ng * QP * sizeof(int));
    p->o_gprefix = off; off = align_up(off + ng * QP * sizeof(float));
    p->o_gllpre = off;  off = align_up(off + ng * sizeof(double));
    p->o_gsuffix = off; off = align_up(off + ng * QP * sizeof(float));
    p->o_glsuf = off;   off = align_up(off + ng * sizeof(double));
    // alpha_hat checkpoints, one QP-float row per (chain, SUB-step block), stored wave by wave:
    // [apply wave][block][chain in wave][QP] — a wave writes (and later reads) one contiguous
    // 1 KB piece per block.  Sized for the scan plan's waves and for the serial exact-clamp plan's
    // (make_xplan: one chunk of ceil(L/16)*16 steps per sequence), which reuses the region.
    p->o_ckpt = off;
    if (op == HMM_OP_POSTERIOR) {
        const size_t scan_rows = (size_t)(((long long)p->b * p->C + 15) / 16) * 16 * p->nsub;
        const size_t exact_rows = (size_t)((p->b + 15) / 16) * 16 * (size_t)(((p->L + 15) / 16) * 16 / SUB);
        off = align_up(off + (size_t)p->k * (scan_rows > exact_rows ? scan_rows : exact_rows) * QP * sizeof(float));
    }
    p->total = off;
    return HMM_OK;
}

// The plan of the serial exact-clamp kernels for the same problem: ONE chunk per sequence, walked
// by the apply kernels with the cell's exact step semantics, 16 sequences per wave.  It shares the
// scan plan's workspace (flags, log-likelihoods; its checkpoints nest inside the scan plan's
// region: NB * ceil(L/16)*2 rows <= nchains * nsub rows).  The apply kernels address a wave's
// chains with 32-bit byte offsets from the wave's base, so 16 whole sequences must span < 2 GB;
// beyond that a wave takes a single sequence.
static int make_xplan(const Plan &p, Plan *x) {
    *x = p;
    x->T = ((p.L + 15) / 16) * 16;
    x->C = 1;
    x->nsub = x->T / SUB;
    x->nchains = p.NB;
    x->G = 0; x->gsize = 0;
    const long long seq_bytes = (long long)x->T * p.q * (long long)sizeof(float);
    x->cpw = 16 * seq_bytes < (1ll << 31) - 4096 ? 16 : 1;
    if (opt(HMM_OPT_EXACT) == HMM_EXACT_ALWAYS_NARROW) x->cpw = 1;     // test hook: the very-long-sequence layout at any size
    if (seq_bytes >= (1ll << 31) - 4096) return HMM_ERR_BAD_SHAPE;      // one sequence of more than 2 GB
    return HMM_OK;
}

// ------------------------------------------------------------------ device helpers

__device__ __forceinline__ f4 mfma4(const float (&a)[4], f4 x) {
    const f4 z = {0.f, 0.f, 0.f, 0.f};
    f4 d = __builtin_amdgcn_mfma_f32_16x16x4f32(a[0], x.x, z, 0, 0, 0);
    d = __builtin_amdgcn_mfma_f32_16x16x4f32(a[1], x.y, d, 0, 0, 0);
    d = __builtin_amdgcn_mfma_f32_16x16x4f32(a[2], x.z, d, 0, 0, 0);
    d = __builtin_amdgcn_mfma_f32_16x16x4f32(a[3], x.w, d, 0, 0, 0);
    return d;
}

// the same product with vector operands and an accumulator: c += Aop(a) * Bop(x)
__device__ __forceinline__ f4 mfma4v(f4 a, f4 x, f4 c) {
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, x.x, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, x.y, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, x.z, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, x.w, c, 0, 0, 0);
    return c;
}

// sum / max over the four lanes (n, n+16, n+32, n+48) that hold one tile column.
// gfx950's v_permlane16_swap / v_permlane32_swap exchange 16- / 32-lane rows between two
// VGPRs in the VALU: with both operands = v the two results are v's even and odd rows
// broadcast pairwise, so their sum is the xor-16 (xor-32) butterfly — no LDS round trip and
// no s_waitcnt in the recurrence's dependency chain (ds_bpermute costs two of each per step).
// Inline asm because this toolchain's __builtin_amdgcn_permlane{16,32}_swap alias their two
// results (verified wrong on hardware); "s_nop 1" covers the VALU-write -> permlane-read hazard.
__device__ __forceinline__ void swap16(float &a, float &b) {
    asm("s_nop 1\n\tv_permlane16_swap_b32_e32 %0, %1" : "+v"(a), "+v"(b));
}
__device__ __forceinline__ void swap32(float &a, float &b) {
    asm("s_nop 1\n\tv_permlane32_swap_b32_e32 %0, %1" : "+v"(a), "+v"(b));
}
__device__ __forceinline__ float col_sum(float v) {
    float a = v, b = v;
    swap16(a, b);
    a += b; b = a;
    swap32(a, b);
    return a + b;
}
// two independent column sums at once: three swaps and two adds where two col_sum take four and four.
// (u_i, w_i: the values in 16-lane row i)  swap16(u, w) leaves [u0 w0 u2 w2] and [u1 w1 u3 w3], their sum is
// [u0+u1 w0+w1 u2+u3 w2+w3]; swap32 of that with itself and the add give [U W U W] with U = (u0+u1) + (u2+u3),
// the association of col_sum, so the bits are col_sum's; the last swap16 spreads U and W over all rows.
__device__ __forceinline__ void col_sum2(float u, float w, float &su, float &sw) {
    swap16(u, w);
    float c = u + w, d = c;
    swap32(c, d);
    float e = c + d, f = e;
    swap16(e, f);
    su = e; sw = f;
}
__device__ __forceinline__ float col_max(float v) {
    float a = v, b = v;
    swap16(a, b);
    a = fmaxf(a, b); b = a;
    swap32(a, b);
    return fmaxf(a, b);
}
__device__ __forceinline__ float hsum(f4 v) { return (v.x + v.y) + (v.z + v.w); }
__device__ __forceinline__ float hmax(f4 v) { return fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w)); }

__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void *base, unsigned long long bytes) {
    unsigned n = bytes > 0xFFFFFFF0ull ? 0xFFFFFFF0u : (unsigned)bytes;
    return __builtin_amdgcn_make_buffer_rsrc((void *)base, 0, (int)n, 0x00020000);
}
// Load N consecutive rows' states 4g..4g+3 for this lane: one 16-byte buffer load per row
// at 4-byte alignment.  Elements past a row's q states are the next row's first values (or,
// at the very end of the tensor, out of the descriptor's range: gfx950 range-checks raw
// buffer accesses per dword and returns 0 there — verified on hardware); clampE() zeroes
// them either way, so no byte outside the (k,b,L,q) tensor is ever dereferenced.
template <int N>
__device__ __forceinline__ void ld_rows(__amdgpu_buffer_rsrc_t r, int voff, int rowb, f4 (&e)[N]) {
#pragma unroll
    for (int s = 0; s < N; ++s)
        e[s] = __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(r, voff + s * rowb, 0, HMM_LD_AUX));
}

// per-lane clamp bounds: valid state -> [eps, +inf), padded state -> [0, 0]
struct Bounds { f4 lo, hi; };
__device__ __forceinline__ Bounds make_bounds(int g, int q, float eps) {
    Bounds bd;
    const float inf = __builtin_inff();
    bd.lo.x = (4 * g + 0 < q) ? eps : 0.f;  bd.hi.x = (4 * g + 0 < q) ? inf : 0.f;
    bd.lo.y = (4 * g + 1 < q) ? eps : 0.f;  bd.hi.y = (4 * g + 1 < q) ? inf : 0.f;
    bd.lo.z = (4 * g + 2 < q) ? eps : 0.f;  bd.hi.z = (4 * g + 2 < q) ? inf : 0.f;
    bd.lo.w = (4 * g + 3 < q) ? eps : 0.f;  bd.hi.w = (4 * g + 3 < q) ? inf : 0.f;
    return bd;
}
__device__ __forceinline__ f4 clampE(f4 e, const Bounds &bd) {
    f4 r;
    r.x = __builtin_amdgcn_fmed3f(e.x, bd.lo.x, bd.hi.x);
    r.y = __builtin_amdgcn_fmed3f(e.y, bd.lo.y, bd.hi.y);
    r.z = __builtin_amdgcn_fmed3f(e.z, bd.lo.z, bd.hi.z);
    r.w = __builtin_amdgcn_fmed3f(e.w, bd.lo.w, bd.hi.w);
    return r;
}
__device__ __forceinline__ f4 fmax4(f4 v, float s) {
    f4 r = {fmaxf(v.x, s), fmaxf(v.y, s), fmaxf(v.z, s), fmaxf(v.w, s)};
    return r;
}
__device__ __forceinline__ f4 sel4(bool c, f4 a, f4 b) { return c ? a : b; }

// MFMA A-operands for lane (g, n).  fwd: Aop = A^T (dst n <- src 4g+kk);  bwd: Aop = A.
__device__ __forceinline__ void load_A(const float *A, int q, int g, int n, float (&af)[4], float (&ab)[4]) {
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
        int s = 4 * g + kk;
        bool ok = (s < q) && (n < q);
        af[kk] = ok ? A[s * q + n] : 0.f;
        ab[kk] = ok ? A[n * q + s] : 0.f;
    }
}

// ------------------------------------------------------------------ reduce

// One wave per (sequence, chunk).  ops[chain][i][k] (i = state at the chunk's last step,
// k = state just before the chunk), exps[chain][k].
__device__ __forceinline__ void reduce_chain(const float *__restrict__ A, const float *__restrict__ E,
                                             float *__restrict__ ops, int *__restrict__ exps,
                                             const int *__restrict__ topo, const Plan &p, float eps, long long chain) {
    const int lane = threadIdx.x & 63, g = lane >> 4, n = lane & 15;
    const int seq = (int)(chain / p.C), c = (int)(chain - (long long)seq * p.C);
    const int m = seq / p.b;
    if (topo && topo[m] != 0) return;      // this model's A fits a sparse topology: k_reduce_sparse has it
    const int t0 = c * p.T;
    const int len = min(p.T, p.L - t0);
    const int q = p.q;

    float af[4], ab[4];
    load_A(A + (size_t)m * q * q, q, g, n, af, ab);
    const Bounds bd = make_bounds(g, q, eps);

    const float *base = E + ((size_t)seq * p.L + t0) * q;
    const __amdgpu_buffer_rsrc_t rs = make_rsrc(base, (unsigned long long)len * q * sizeof(float));
    const int rowb = q * (int)sizeof(float);
    int voff = g * 16;

    f4 X;
    X.x = (4 * g + 0 == n) ? 1.f : 0.f;
    X.y = (4 * g + 1 == n) ? 1.f : 0.f;
    X.z = (4 * g + 2 == n) ? 1.f : 0.f;
    X.w = (4 * g + 3 == n) ? 1.f : 0.f;
    int ex = 0;        // column n holds X[:,n] * 2^-ex

    // The operator is the exactly linear product of the steps A diag(max(E, eps)): the cell's clamp of
    // the state MIXTURE (MsaHmmCell.py:88) has no per-column form, and leaving it out is what keeps the
    // scan closest to the serial recursion (its whole deviation is the posterior mass of clamp-born
    // paths, which the apply kernels measure: see backward_body's psi).
    // rescale the column by the power of two that brings its sum into [0.5, 1): exact
    auto rescale = [&](f4 &V) {
        float s = col_sum(hsum(V));
        int xe = __builtin_amdgcn_frexp_expf(s);
        float sc = __builtin_amdgcn_ldexpf(1.0f, -xe);     // exact power of two
        V = V * sc;
        ex += xe;
    };

    int t = 0;
    if (c == 0 && p.seq_start) {   // first observation of the sequence: no transition (MsaHmmCell.py:78-79)
        f4 e0[1];
        ld_rows<1>(rs, voff, rowb, e0);
        X = X * clampE(e0[0], bd);
        rescale(X);
        voff += rowb;
        t = 1;
    }
    // software-pipelined emission stream: HMM_REDUCE_PF rows in flight ahead of the recurrence
    constexpr int PF = HMM_REDUCE_PF;
    f4 en[PF];
    ld_rows<PF>(rs, voff, rowb, en);
    for (; t < len; t += PF) {
        f4 ec[PF];
#pragma unroll
        for (int u = 0; u < PF; ++u) ec[u] = en[u];
        voff += PF * rowb;
        ld_rows<PF>(rs, voff, rowb, en);
#pragma unroll
        for (int u = 0; u < PF; ++u) {
            if (t + u < len) {          // wave-uniform
                X = mfma4(af, X) * clampE(ec[u], bd);
                rescale(X);
            }
        }
    }
    float *o = ops + (size_t)chain * QP * QP;
    o[(4 * g + 0) * QP + n] = X.x;
    o[(4 * g + 1) * QP + n] = X.y;
    o[(4 * g + 2) * QP + n] = X.z;
    o[(4 * g + 3) * QP + n] = X.w;
    if (g == 0) exps[(size_t)chain * QP + n] = ex;
}

// Waves walk the chains with a grid stride: when every model is served by a sparse-topology kernel
// (decided on the device) the launch costs a few thousand blocks that find nothing to do, not one
// block per four chains (27 us at 200 000 chains).
__global__ __launch_bounds__(256) void k_reduce(const float *__restrict__ A, const float *__restrict__ E,
                                                float *__restrict__ ops, int *__restrict__ exps,
                                                const int *__restrict__ topo, Plan p, float eps) {
    const long long stride = (long long)gridDim.x * 4;
    for (long long chain = (long long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
         chain < p.nchains; chain += stride)
        reduce_chain(A, E, ops, exps, topo, p, eps, chain);
}

// ------------------------------------------------------------------ reduce, sparse topologies

// The gene-prediction models' A has 23 (15-state) / 15 (7-state) non-zeros.  On gfx950 the f32
// MFMA runs on the FP32 vector lanes (it does not overlap VALU work: measured per-step cost =
// 4 x 32 MFMA cycles + 4 x #VALU), so for a known support it is cheaper to keep one operator
// COLUMN per lane (15 registers) and do only the structural non-zero fma's: lane = (chain,
// start state), 4 chains per wave, ~70 VALU per 4 positions instead of 4 MFMA + ~33 VALU per
// position.  Results (ops/exps) have the dense kernel's format.  Which kernel serves a model is
// decided on the device from A itself (k_topo_check): the dense MFMA kernel stays the generic path.

struct TopoGene15 {      // hmm_layer/gene_pred_hmm_transitioner.py:200-221, 279-303 (k = 1)
    static constexpr int Q = 15, NE = 23, ID = 1;
    // CSR by destination state: sources of state j are src[start[j] .. start[j+1])
    static constexpr int start[Q + 1] = {0, 2, 4, 6, 8, 10, 13, 15, 16, 17, 18, 19, 20, 21, 22, 23};
    static constexpr int src[NE] = {0, 14, 8, 1, 9, 2, 10, 3, 11, 6, 7, 4, 12, 5, 13, 0, 4, 5, 6, 1, 2, 3, 5};
};
struct TopoGene7 {       // hmm_layer/gene_pred_hmm_transitioner.py:132-148
    static constexpr int Q = 7, NE = 15, ID = 2;
    static constexpr int start[Q + 1] = {0, 2, 4, 6, 8, 11, 13, 15};
    static constexpr int src[NE] = {0, 6, 4, 1, 5, 2, 6, 3, 0, 6, 3, 4, 1, 5, 2};
};

struct TopoGene29 {      // two copies of the 14 gene states around one intergenic state:
                         // hmm_layer/gene_pred_hmm_transitioner.py:263-308 (GenePredMultiHMMTransitioner, k = 2)
    static constexpr int Q = 29, NE = 45, ID = 3;
    static constexpr int start[Q + 1] = {0, 3, 5, 7, 9, 11, 13, 15, 17, 19, 22, 25, 27, 29, 30, 31, 32, 33, 34, 35, 36,
                                         37, 38, 39, 40, 41, 42, 43, 44, 45};
    static constexpr int src[NE] = {0, 27, 28, 15, 1, 16, 2, 17, 3, 18, 4, 19, 5, 20, 6, 21, 11, 22, 12, 13, 7, 23, 14,
                                    8, 24, 9, 25, 10, 26, 0, 0, 7, 8, 9, 10, 11, 12, 1, 2, 3, 4, 5, 6, 9, 10};
};

// number of edges of T that leave state i
template <class T>
__host__ __device__ constexpr int out_degree(int i) {
    int n = 0;
    for (int e = 0; e < T::NE; ++e) n += (T::src[e] == i) ? 1 : 0;
    return n;
}
// Every state of T with a single outgoing edge carries weight exactly 1 on it in A (what a softmax over
// one edge gives: the gene models' START, EI, IE and STOP states): k_reduce_sparse then never forms
// x_i = y_i * e_i for those states but feeds (e_i, y_i) straight into the successor's fma.
#define TOPO_UNIT 16
// A pass-through state has exactly one incoming and one outgoing edge (START, EI, IE, STOP): with weight 1 on the
// way out (TOPO_UNIT) it is a pure one-step delay, and the unit-weight sparse reduce runs a second-order recurrence
// on the remaining (live) states that never forms it (HMM_RS_ORDER2, reduce_sparse_wave).
template <class T>
__host__ __device__ constexpr bool passthrough(int j) {
    return T::start[j + 1] - T::start[j] == 1 && out_degree<T>(j) == 1;
}
template <class T>
__host__ __device__ constexpr int pt_src(int p) { return T::src[T::start[p]]; }      // the one state that feeds p
template <class T>
__host__ __device__ constexpr int pt_dst(int p) {                                     // the one state p feeds
    for (int j = 0; j < T::Q; ++j)
        for (int e = T::start[j]; e < T::start[j + 1]; ++e)
            if (T::src[e] == p) return j;
    return -1;
}
template <class T>
__host__ __device__ constexpr int n_passthrough() {
    int n = 0;
    for (int j = 0; j < T::Q; ++j) n += passthrough<T>(j) ? 1 : 0;
    return n;
}
// both neighbours of every pass-through state are live: delays do not chain, the recurrence has order two
template <class T>
__host__ __device__ constexpr bool passthrough_between_live() {
    for (int p = 0; p < T::Q; ++p)
        if (passthrough<T>(p) && (passthrough<T>(pt_src<T>(p)) || passthrough<T>(pt_dst<T>(p)))) return false;
    return true;
}
static_assert(n_passthrough<TopoGene15>() == 8 && passthrough_between_live<TopoGene15>(), "15-state gene model: 7 live states");
static_assert(n_passthrough<TopoGene29>() == 16 && passthrough_between_live<TopoGene29>(), "29-state gene model: 13 live states");
static_assert(n_passthrough<TopoGene7>() == 0, "the 7-state model has no pass-through state");
// entry (i -> j) of A lies inside topology T's support
template <class T>
__device__ __forceinline__ bool edge_in(int i, int j) {
    bool ok = false;
    for (int e = T::start[j]; e < T::start[j + 1]; ++e) ok = ok || (T::src[e] == i);
    return ok;
}

// topo[m] = ID of the sparse topology that contains the support of A[m], 0 = none (dense kernel),
// TOPO_EXACT = the chunked scan must not serve this model at all.
// One wave per model, lanes over the q*q entries (a single thread walking them took 32 us).
//
// TOPO_EXACT.  The cell clamps the predicted state mixture at eps every step
// (hmm_layer/MsaHmmCell.py:87-88); chunk operators can only floor each conditional column, which is
// the same thing up to O(eps) as long as no state's mass ever lives on the floor alone.  When the
// support of A (entries > eps: a smaller entry cannot lift its target above the clamp) is not
// PRIMITIVE — reducible chains, A = I, periodic chains, states without incoming edges, all-zero
// rows as in the reference's as-shipped matrices (hmm_layer/Transitioner.py:366-367) — forward
// and backward evidence can contradict each other outright and the answer is decided by the floors:
// those models are served by the serial exact-clamp kernels.  Primitive <=> B^n > 0 for every
// n >= (q-1)^2 + 1 (Wielandt); 8 boolean squarings give B^256, enough for q <= 16.
#define TOPO_EXACT 255
__global__ __launch_bounds__(64) void k_topo_check(const float *__restrict__ A, int *__restrict__ topo, int k, int q,
                                                   int force_dense, int exact_mode, float eps, int *__restrict__ nexact,
                                                   int *__restrict__ wcnt = nullptr) {
    const int m = blockIdx.x;
    const float *Am = A + (size_t)m * q * q;
    if (m == 0 && threadIdx.x == 0) *nexact = 0;
    if (m == 0 && threadIdx.x < 4 && wcnt) wcnt[threadIdx.x] = 0;
    bool exact = exact_mode == HMM_EXACT_ALWAYS || exact_mode == HMM_EXACT_ALWAYS_NARROW;
    if (exact_mode == HMM_EXACT_AUTO) {
        int row = 0;                                            // lane i < q: row i of the support as a bit mask
        if ((int)threadIdx.x < q)
            for (int j = 0; j < q; ++j) row |= (Am[threadIdx.x * q + j] > eps) ? (1 << j) : 0;
        for (int it = 0; it < 8; ++it) {
            int nr = 0;
            for (int j = 0; j < q; ++j) {
                const int rj = __builtin_amdgcn_readlane(row, j);
                nr |= ((row >> j) & 1) ? rj : 0;
            }
            row = nr;
        }
        const bool notfull = (int)threadIdx.x < q && row != (1 << q) - 1;
        exact = __ballot(notfull) != 0ull;
    }
    if (exact) {
        if (threadIdx.x == 0) topo[m] = TOPO_EXACT;
        return;
    }
    bool bad15 = q != TopoGene15::Q, bad7 = q != TopoGene7::Q;
    bool nonunit15 = false, nonunit7 = false;      // an edge out of a single-successor state that is not exactly 1
    if (!force_dense && (!bad15 || !bad7))
        for (int e = threadIdx.x; e < q * q; e += 64) {
            const float a = Am[e];
            const int i = e / q, j = e - i * q;
            if (!bad15) {
                const bool in = edge_in<TopoGene15>(i, j);
                bad15 = a != 0.f && !in;
                nonunit15 = nonunit15 || (in && a != 1.0f && out_degree<TopoGene15>(i) == 1);
            }
            if (!bad7) {
                const bool in = edge_in<TopoGene7>(i, j);
                bad7 = a != 0.f && !in;
                nonunit7 = nonunit7 || (in && a != 1.0f && out_degree<TopoGene7>(i) == 1);
            }
        }
    // (lanes over the entries: a single lane walking the topology's edges for the unit test took 10 of the
    // kernel's 20 us — a tenth of a whole log-likelihood call at b = 256 x L = 1e4)
    const bool any15 = __ballot(bad15) != 0ull, any7 = __ballot(bad7) != 0ull;
    const bool nu15 = __ballot(nonunit15) != 0ull, nu7 = __ballot(nonunit7) != 0ull;
    if (threadIdx.x == 0) {
        int id = force_dense ? 0 : (!any15 ? TopoGene15::ID : (!any7 ? TopoGene7::ID : 0));
        if (id == TopoGene15::ID && !nu15) id |= TOPO_UNIT;
        if (id == TopoGene7::ID && !nu7) id |= TOPO_UNIT;
        topo[m] = id;
    }
}

#define SP_TILE 16     // steps staged per LDS tile

#ifndef HMM_RS_AHEAD
#define HMM_RS_AHEAD 0     // sparse reduce: read each step's emission row from LDS one step ahead (A/B: the
                           // registers are worth more as a fourth wave per SIMD: 2.10 -> 2.00 ms with HMM_RS_WPE 4)
#endif
#ifndef HMM_RS_UNI
#define HMM_RS_UNI 1       // sparse reduce: wave-uniform transition weights in SGPRs when the wave holds one model
#endif
#ifndef HMM_POST_BLOCK
#define HMM_POST_BLOCK 16  // block length (checkpoint spacing) of hmm_posterior's scan-plan pair in probability mode
#endif
#ifndef HMM_RS_SUM2
#define HMM_RS_SUM2 1      // sparse reduce: the column sum (and the rescale test) every second step
#endif
#ifndef HMM_RS_ORDER2
#define HMM_RS_ORDER2 1    // sparse reduce, unit-weight wave of one model: second-order recurrence on the live states
                           // (the pass-through states' incoming weight folded into the staged emission)
#endif
#ifndef HMM_RS_QUADROW
#define HMM_RS_QUADROW 0   // sparse reduce, second-order step with 16 lanes per chain: a lane reads 4 floats of a step's row,
                           // the four lanes of a DPP quad hold the row between them (quad_mul / quad_fmac): one 16-byte LDS
                           // read per step where a lane that reads the whole row for itself takes four.  Bit-identical
                           // results, a quarter of the LDS reads, 19 % fewer vector instructions per tile with the gate
                           // below, and slower: 1.40 ms against 1.35 with the gate alone, 1.61 against 1.41 without it
                           // (the compiler pads every use of an asm result by the next instruction with an s_nop)
#endif
#ifndef HMM_RS_SUMGATE
#define HMM_RS_SUMGATE 1   // sparse reduce, same path: the column sum only where the largest live entry of some column
                           // is below the rescale threshold (A/B: 1.33-1.42 -> 1.28-1.37 ms, faster in each of six rounds)
#endif
#ifndef HMM_RS_ROW128
#define HMM_RS_ROW128 1    // sparse reduce: read a staged row's last three floats together with the pad float: a 16-byte
                           // LDS read takes 4 LDS cycles per wave, a 12-byte one 8 (A/B: 1.47-1.51 -> 1.37-1.43 ms)
#endif
#ifndef HMM_RS_WPE
#define HMM_RS_WPE 4       // waves per SIMD the register allocator of the 16-lane sparse reduce is held to (0: its own choice)
#endif
#if HMM_RS_WPE
#define RS_ATTR __attribute__((amdgpu_waves_per_eu(HMM_RS_WPE, HMM_RS_WPE)))
#else
#define RS_ATTR
#endif
// Lane layout of the sparse reduce: W lanes per chain (the padded state count: 16, or 32 for the 29-state
// model), 64 / W chains per wave.  One wave's staging: [buffer][chain in wave][step x W floats (+pad)].
template <class T> struct RsCfg {
    static constexpr int W = T::Q <= 16 ? 16 : 32;
    static constexpr int CPW = 64 / W;
    static constexpr int PIECES = SP_TILE * T::Q / 4;        // 16-byte pieces of one chain's 16-step tile
    static constexpr int RPC = (PIECES + 63) / 64;           // load rounds per chain per tile
    typedef float Lds[2][CPW][SP_TILE * W + 16];
};

// HMM_RS_QUADROW.  Lane kc of a chain holds floats 4(kc&3) .. 4(kc&3)+3 of a staged row in `r`: float j is component
// j&3 of quad lane j>>2, the same in all four quads of the chain.  A VOP2 instruction takes it from there as its DPP
// source operand, so row[j] * v and acc + row[j] * v stay ONE instruction each, the same multiply / fma on the same
// numbers as with the row in the lane's own registers.  (The compiler folds __builtin_amdgcn_update_dpp into a
// multiply but not into a v_fmac: it keeps a v_mov_b32_dpp in front of each.)  The hardware wants two instructions
// between a VALU write of a register and its use as DPP source, and the compiler does not look inside the asm string:
// the row registers are written by the LDS read alone and never copied (reduce_sparse_wave keeps two sets and unrolls
// the step pair).  The other two operands are ordinary reads.  What the compiler does do is pad a use of an asm result
// by the very next instruction with an s_nop 0 (it cannot rule out a partial write), 24 per 16-step tile: see
// HMM_RS_QUADROW's A/B.
// All four lanes of a quad are active wherever these run: lanes leave the step loop a whole chain at a time.
#define RS_QUAD_OP(op, ql, ...) \
    asm(op " %0, %1, %2 quad_perm:[" #ql "," #ql "," #ql "," #ql "] row_mask:0xf bank_mask:0xf" : __VA_ARGS__)
__device__ __forceinline__ float quad_mul(const f4 &r, int j, float v) {            // row[j] * v
    float d;
    switch (j >> 2) {
    case 0: RS_QUAD_OP("v_mul_f32_dpp", 0, "=v"(d) : "v"(r[j & 3]), "v"(v)); break;
    case 1: RS_QUAD_OP("v_mul_f32_dpp", 1, "=v"(d) : "v"(r[j & 3]), "v"(v)); break;
    case 2: RS_QUAD_OP("v_mul_f32_dpp", 2, "=v"(d) : "v"(r[j & 3]), "v"(v)); break;
    default: RS_QUAD_OP("v_mul_f32_dpp", 3, "=v"(d) : "v"(r[j & 3]), "v"(v)); break;
    }
    return d;
}
__device__ __forceinline__ float quad_fmac(const f4 &r, int j, float v, float acc) { // fma(row[j], v, acc)
    switch (j >> 2) {
    case 0: RS_QUAD_OP("v_fmac_f32_dpp", 0, "+v"(acc) : "v"(r[j & 3]), "v"(v)); break;
    case 1: RS_QUAD_OP("v_fmac_f32_dpp", 1, "+v"(acc) : "v"(r[j & 3]), "v"(v)); break;
    case 2: RS_QUAD_OP("v_fmac_f32_dpp", 2, "+v"(acc) : "v"(r[j & 3]), "v"(v)); break;
    default: RS_QUAD_OP("v_fmac_f32_dpp", 3, "+v"(acc) : "v"(r[j & 3]), "v"(v)); break;
    }
    return acc;
}
// a row as the step takes it: Q floats of the lane's own, or the quad's four registers
__device__ __forceinline__ float row_mul(const f4 &r, int j, float v) { return quad_mul(r, j, v); }
__device__ __forceinline__ float row_fma(const f4 &r, int j, float v, float acc) { return quad_fmac(r, j, v, acc); }
template <int N> __device__ __forceinline__ float row_mul(const float (&r)[N], int j, float v) { return r[j] * v; }
template <int N> __device__ __forceinline__ float row_fma(const float (&r)[N], int j, float v, float acc) {
    return fmaf(r[j], v, acc);
}

// UNIT: every single-out-edge state of T has weight 1 on its edge (TOPO_UNIT, for all of the wave's chains)
//       With UNI as well, and pass-through states in T, the wave runs the second-order recurrence (HMM_RS_ORDER2).
// UNI:  all chains of the wave belong to one model (always, unless k > 1 and the wave straddles two): the
//       transition weights are then wave-uniform and live in SGPRs — 15 to 23 vector registers that the column
//       and the emission row need (held to 128 VGPRs for four waves per SIMD, the kernel spilled 26 dwords)
template <class T, bool UNIT, bool UNI>
__device__ __forceinline__ void reduce_sparse_wave(const float *__restrict__ A, const float *__restrict__ E,
                                                   float *__restrict__ ops, int *__restrict__ exps, const Plan &p,
                                                   float eps, typename RsCfg<T>::Lds &ldsw, long long wchain0,
                                                   bool mine, int m, long long chain, int c) {
    constexpr int Q = T::Q, W = RsCfg<T>::W, CPW = RsCfg<T>::CPW, RPC = RsCfg<T>::RPC;
    // O2: the second-order recurrence on the live states (see `step`); needs unit weights out of the pass-through
    // states and ONE model per wave, whose incoming weights are folded into the staged emissions
    constexpr bool O2 = HMM_RS_ORDER2 && UNIT && UNI && n_passthrough<T>() > 0;
    static_assert(!O2 || passthrough_between_live<T>(), "a pass-through state between two live states");
    // QR: a step's emission row in the four lanes of a quad (HMM_RS_QUADROW); GATE: the column sum on demand
    constexpr bool QR = HMM_RS_QUADROW && O2 && W == 16, GATE = HMM_RS_SUMGATE && O2 && W == 16;
    auto live = [](int j) constexpr { return !O2 || !passthrough<T>(j); };
    const int lane = threadIdx.x & 63, cl = lane / W, kc = lane % W;
    const int t0 = c * p.T;
    const int len = mine ? min(p.T, p.L - t0) : 0;
    const bool first = (c == 0) && p.seq_start;

    // transition weights of this lane's model, one per structural non-zero
    float a[T::NE];
    {
        const float *Am = A + (size_t)(UNI ? __builtin_amdgcn_readfirstlane(m) : m) * Q * Q;
#pragma unroll
        for (int j = 0; j < Q; ++j)
#pragma unroll
            for (int e = T::start[j]; e < T::start[j + 1]; ++e) a[e] = Am[T::src[e] * Q + j];
    }

    // ---- emission staging: the wave's 4 chains are adjacent in memory; each chain's 16-step
    // tile is 16*Q contiguous floats = (16*Q*4/16) 16-byte pieces, one per lane
    const int seq0 = (int)(wchain0 / p.C), c0 = (int)(wchain0 - (long long)seq0 * p.C);
    const long long row0 = (long long)seq0 * p.L + (long long)c0 * p.T;
    const unsigned long long total = (unsigned long long)p.NB * p.L * Q * sizeof(float);
    const __amdgpu_buffer_rsrc_t rs = make_rsrc(E + row0 * Q, total - (unsigned long long)row0 * Q * sizeof(float));
    constexpr int PIECES = RsCfg<T>::PIECES;               // 60 for Q = 15, 28 for Q = 7, 116 for Q = 29
    static_assert(SP_TILE * Q % 4 == 0, "tile must be a whole number of 16-byte pieces");
    int coff[CPW];                                          // byte offset of chain j's chunk from the wave base
#pragma unroll
    for (int j = 0; j < CPW; ++j) {
        long long ch = wchain0 + j;
        if (ch >= p.nchains) ch = wchain0;
        const long long sq = ch / p.C;
        const long long rw = sq * p.L + (ch - sq * p.C) * (long long)p.T;
        coff[j] = (int)((rw - row0) * Q * (long long)sizeof(float));
    }
    int loff[RPC][4];                                       // where this lane's 4 floats of a piece go in a tile
#pragma unroll
    for (int rr = 0; rr < RPC; ++rr)
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int idx = 4 * (rr * 64 + lane) + u;
            loff[rr][u] = (idx / Q) * W + (idx % Q);
        }
    // O2: the staged value of a pass-through state p is e'_p = max(E[p], eps) * a(src(p) -> p): the state of each of
    // the lane's four floats per piece is fixed, so the factor is a per-lane constant (1 for a live state)
    float smul[O2 ? RPC : 1][4];
    if constexpr (O2) {
#pragma unroll
        for (int rr = 0; rr < RPC; ++rr)
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int st = (4 * (rr * 64 + lane) + u) % Q;
                float mv = 1.f;
#pragma unroll
                for (int pp = 0; pp < Q; ++pp)
                    if (passthrough<T>(pp)) mv = (st == pp) ? a[T::start[pp]] : mv;
                smul[rr][u] = mv;
            }
    }
    for (int i = lane; i < 2 * CPW * (SP_TILE * W + 16); i += 64) (&ldsw[0][0][0])[i] = 0.f;   // pad columns = 0

    f4 r[CPW * RPC];
    auto fetch = [&](int tile) {
#pragma unroll
        for (int j = 0; j < CPW; ++j)
#pragma unroll
            for (int rr = 0; rr < RPC; ++rr)
                r[j * RPC + rr] = __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(
                    rs, coff[j] + tile * (SP_TILE * Q * 4) + (rr * 64 + lane) * 16, 0, 0));
    };
    auto stage = [&](int buf) {
#pragma unroll
        for (int rr = 0; rr < RPC; ++rr) {
            if (rr * 64 + lane < PIECES) {
#pragma unroll
                for (int j = 0; j < CPW; ++j) {
                    float *dst = &ldsw[buf][j][0];
                    const f4 v = r[j * RPC + rr];
                    if constexpr (O2) {
                        dst[loff[rr][0]] = fmaxf(v.x, eps) * smul[rr][0];
                        dst[loff[rr][1]] = fmaxf(v.y, eps) * smul[rr][1];
                        dst[loff[rr][2]] = fmaxf(v.z, eps) * smul[rr][2];
                        dst[loff[rr][3]] = fmaxf(v.w, eps) * smul[rr][3];
                    } else {
                        dst[loff[rr][0]] = fmaxf(v.x, eps);     // the cell's max(E, eps), once per value
                        dst[loff[rr][1]] = fmaxf(v.y, eps);
                        dst[loff[rr][2]] = fmaxf(v.z, eps);
                        dst[loff[rr][3]] = fmaxf(v.w, eps);
                    }
                }
            }
        }
    };

    // x[j]: the column.  UNIT: for a state j with a single outgoing edge x[j] holds the PRE-emission value
    // y_j and pend[j] the emission it still has to be multiplied with (the true entry is x[j] * pend[j]):
    // its only consumer multiplies by a weight of 1, so (pend[j], x[j]) go straight into that fma and the
    // product is never formed — 8 of the 15 emission multiplies of the 15-state model.
    // O2: only the live states have an x[j], the column one step back, and an xb[j], the column two steps back; for
    // a pass-through state p, pend[p] is e'_p of the last row taken and its entry is pend[p] * xb[src(p)], formed
    // only at the column's end.  A column that STARTS in pass-through state p is a unit of mass in flight: this
    // lane alone sees pend[p] = 1 in front of its first step, with xb[src(p)] = 1.
    // QR: the last row taken is the quad's row registers rq[] and there is no pend[] in the loop; a chunk's first
    // two steps, where one lane's weights differ from its neighbours', take a per-lane copy (tile_steps).
    // Everything below that works with "the last row" (`pw`: pass-through weights) or "this step's row" (`e`) takes
    // it in either form, row_mul / row_fma.
    float x[Q], pend[Q], xb[O2 ? Q : 1];
    f4 rq[2] = {f4{0.f, 0.f, 0.f, 0.f}, f4{0.f, 0.f, 0.f, 0.f}};      // QR: rows of the even / the odd steps
    auto flight_src = [&](int i) {       // O2: this lane's start state is a pass-through state fed by state i
        bool f = false;
#pragma unroll
        for (int pp = 0; pp < Q; ++pp)
            if (passthrough<T>(pp) && pt_src<T>(pp) == i) f = f || (kc == pp);
        return f;
    };
    // (QR: the unit column is set up where the chunk's first tile begins, tile_steps_quad: constants here, so that
    // no per-lane value has to be kept from this point through the prologue and both tile loops)
#pragma unroll
    for (int j = 0; j < Q; ++j) {
        x[j] = (!QR && j == kc) ? 1.f : 0.f;
        pend[j] = 1.f;
        if constexpr (O2) {
            pend[j] = x[j];
            xb[j] = (!QR && flight_src(j)) ? 1.f : 0.f;
        }
    }
    int ex = 0;
    float cs = (kc < Q) ? 1.f : 0.f;     // sum of the column as currently scaled
    auto deferred = [](int j) constexpr { return !O2 && UNIT && out_degree<T>(j) == 1; };

    // exact power-of-two rescale of the column (sum back into [0.5, 1)).  The exponent is clamped
    // so that the factor cannot overflow when a column has underflowed to a denormal or to zero
    // (a start state from which the chunk is impossible even through the eps clamps: its weight
    // in the scan is then 0, as it should be).
    // risk: the column's sum has been found below 2^-100 at a rescale — it has then been through the denormal range
    // (two observations in a row that every path survives only at the emission floor take 2^-106 off between two sums)
    // and its entries are no longer good to fp32's precision relative to each other.  Nothing to do with the clamps of
    // the state mixture, so psi does not see it: the chain is marked (pad lane of its exponent row) and k_exact_select
    // treats it as flagged.
    bool risk = false;
    auto rescale = [&]() {
        risk = risk || (kc < Q && cs < 0x1p-100f);
        int xe = max(__builtin_amdgcn_frexp_expf(cs), -100);
        float sc = __builtin_amdgcn_ldexpf(1.0f, -xe);
#pragma unroll
        for (int j = 0; j < Q; ++j) {
            if (live(j)) x[j] *= sc;
            if constexpr (O2) { if (live(j)) xb[j] *= sc; }       // (mass in flight scales through xb)
        }
        cs *= sc;
        ex += xe;
    };

    // finalise and store this lane's operator column (called once, at the lane's last step)
    auto entry = [&](const auto &pw, int j) {            // entry j of the column as it stands
        if constexpr (O2) {
            if (live(j)) return x[j];
            return row_mul(pw, j, xb[pt_src<T>(j)]);
        } else {
            return deferred(j) ? x[j] * pw[j] : x[j];
        }
    };
    auto column_sum = [&](const auto &pw) {
        float s = 0.f;
        if constexpr (O2) {
#pragma unroll
            for (int j = 0; j < Q; ++j) if (live(j)) s += x[j];
#pragma unroll
            for (int j = 0; j < Q; ++j) if (!live(j)) s = row_fma(pw, j, xb[pt_src<T>(j)], s);
        } else {
#pragma unroll
            for (int j = 0; j < Q; ++j) s += entry(pw, j);
        }
        return s;
    };
    auto finish = [&](const auto &pw) {
        const float fs = column_sum(pw);             // (the running sum may be a step old)
        float *o = ops + (size_t)chain * W * W;
        bool frisk;
        int fex;
        if constexpr (QR) {
            // rescale()'s arithmetic on a copy: a lane that has stored its column needs none of its state again, and a
            // wave with a sequence's tail calls this after every step, where each variable written would be one more
            // value to merge (the kernel is held to 128 registers)
            const float fcs = kc < Q ? fs : 0.f;
            frisk = risk || (kc < Q && fcs < 0x1p-100f);
            const int xe = max(__builtin_amdgcn_frexp_expf(fcs), -100);
            const float sc = __builtin_amdgcn_ldexpf(1.0f, -xe);
            fex = ex + xe;
#pragma unroll
            for (int j = 0; j < Q; ++j) {            // (the pad lane takes part: it is a quad's source lane)
                const float ent = live(j) ? x[j] * sc : row_mul(pw, j, xb[pt_src<T>(j)] * sc);
                o[j * W + kc] = (kc < Q) ? ent : 0.f;
            }
        } else {
            cs = kc < Q ? fs : 0.f;
            rescale();
            frisk = risk;
            fex = ex;
#pragma unroll
            for (int j = 0; j < Q; ++j) o[j * W + kc] = (kc < Q) ? entry(pw, j) : 0.f;
        }
#pragma unroll
        for (int j = Q; j < W; ++j) o[j * W + kc] = 0.f;
        static_assert(Q < W, "the exponent row's last lane is a pad lane");
        const unsigned long long rb = __builtin_amdgcn_ballot_w64(frisk) >> (W == 64 ? 0 : W * cl);
        const bool chain_risk = (W == 64 ? rb : (rb & ((1ull << (W & 63)) - 1ull))) != 0ull;
        exps[(size_t)chain * W + kc] = (kc < Q) ? fex : ((kc == W - 1 && chain_risk) ? 1 : 0);
    };
    // one recurrence step on the column: x <- max(E,eps) * (A^T x): exactly linear.  (Rounds 1-2 added
    // eps * sum(x) to every state, a per-column stand-in for the cell's clamp of the state mixture; on the
    // gene models' own emissions that floor costs more accuracy than it buys — the floored scan is off by
    // eps * sum_t 1/<alpha_hat_t, R_t>, up to 1.6e-4 in a posterior for peaked class probabilities, the
    // floor-free one by the posterior mass of clamp-born paths, 1e-8 .. 1e-7 there; tools/experiments/cert_study.py.)
    // e: the clamped emission row of this step, already in registers
    // SUM (compile-time): also form the column's sum and rescale if it has become small; the callers ask for it
    // every second step — the sum is 15 of a step's 48 instructions and nothing but the rescaling needs it since
    // the operators carry no floor.  From the threshold two steps of the smallest emissions a realistic path
    // sees (2^-32: a free state's 1/4096 times a class probability of 1e-6) stay normal numbers; a column that
    // loses more than that in two steps has met two impossible observations and weighs nothing.
    //
    // O2.  A pass-through state p only delays its source's mass by a step: x_p(t) = e_p(t) a(i->p) x_i(t-1), all of
    // which moves on to p's one successor with weight 1.  With e'_p = e_p a(i->p) staged once per emission value
    // (the product is the same for all Q columns of a chain) the live states obey
    //     y_j(t) = sum_{live i->j} a_ij x_i(t-1)  +  sum_{p->j} e'_p(t-1) x_src(p)(t-2),      x_j(t) = y_j(t) e_j(t)
    // 15-state model: 7 multiplies + 8 fma's + 7 emission multiplies = 22 per step for 30, and no pass-through
    // value inside the loop.  The true column sum is sum_live x_j(t) + sum_p e'_p(t) x_src(p)(t-1): the same number
    // as before, so threshold, risk mark and the argument above stand; x and xb take the same power of two.
    //
    // pw: the last row taken (pend[], or the quad's registers of the step before), e: this step's row in the same form.
    // GATE.  The sum is formed only to ask whether some column of the wave has fallen below 2^-40, and every entry is
    // a product of non-negative numbers: each rounded add or fma of the sum returns at least its non-negative addend
    // (rounding is monotonic and the addend is a float), so the sum as computed is at least the largest live entry.
    // Where that is 2^-40 or more in every column the test below cannot fire and the sum is not formed; cs then
    // stays stale, and it is read by rescale() alone, after being set on the slow path or in finish().  Rescale points,
    // exponents and the risk mark are therefore the ungated ones.  A dead column only costs speed: a lane whose live
    // entries are all exactly zero sends its wave through the full sum every time (and, as before, never rescales it).
    auto step = [&](auto &pw, const auto &e, auto sumc) {
        constexpr bool SUM = decltype(sumc)::value;
        float y[Q];
        float s = 0.f;
        bool need = true;
        if constexpr (O2) {
#pragma unroll
            for (int j = 0; j < Q; ++j) {
                if (!live(j)) continue;
                float acc = 0.f;
                bool any = false;
#pragma unroll
                for (int pass = 0; pass < 2; ++pass)            // the direct edges first, then the delayed ones
#pragma unroll
                    for (int ed = T::start[j]; ed < T::start[j + 1]; ++ed) {
                        const int i = T::src[ed];
                        if (live(i) != (pass == 0)) continue;
                        if (live(i)) acc = any ? fmaf(a[ed], x[i], acc) : a[ed] * x[i];
                        else if (any) acc = row_fma(pw, i, xb[pt_src<T>(i)], acc);
                        else acc = row_mul(pw, i, xb[pt_src<T>(i)]);
                        any = true;
                    }
                y[j] = acc;
            }
#pragma unroll
            for (int j = 0; j < Q; ++j) {
                if (live(j)) { xb[j] = x[j]; x[j] = row_mul(e, j, y[j]); }
                else if constexpr (!std::is_same<typename std::decay<decltype(e)>::type, f4>::value) pw[j] = e[j];
            }
            if constexpr (SUM && GATE) {
                float mx = 0.f;
                bool anym = false;
#pragma unroll
                for (int j = 0; j < Q; ++j)
                    if (live(j)) { mx = anym ? fmaxf(mx, x[j]) : x[j]; anym = true; }
                // 0 counts as small; the pad lanes (kc >= Q, all-zero columns) are masked out of the ballot
                constexpr unsigned long long COLS = ((1ull << (Q & 15)) - 1ull) * 0x0001000100010001ull;   // W == 16
                need = (__builtin_amdgcn_ballot_w64(!(mx >= 0x1p-40f)) & COLS) != 0ull;
            }
            if (SUM && need) s = column_sum(e);
        } else {
#pragma unroll
            for (int j = 0; j < Q; ++j) {
                float acc = 0.f;
#pragma unroll
                for (int ed = T::start[j]; ed < T::start[j + 1]; ++ed) {
                    const int i = T::src[ed];
                    const float w = deferred(i) ? pw[i] : a[ed];             // weight 1: the pending emission instead
                    acc = (ed == T::start[j]) ? w * x[i] : fmaf(w, x[i], acc);
                }
                y[j] = acc;
            }
#pragma unroll
            for (int j = 0; j < Q; ++j) {
                if (SUM) s = fmaf(y[j], e[j], s);
                if (deferred(j)) { x[j] = y[j]; pw[j] = e[j]; }
                else x[j] = y[j] * e[j];
            }
        }
        if (SUM && need) {
            // (32-lane rows — the 29-state model: a column that loses more than 2^-45 between two sums has met an
            // observation that everything survives at the emission floor only; such sequences go to the serial kernels,
            // k_scan_select, on top of the certificates of the 32-state apply kernels)
            if (W >= 32) {                      // ... EVERY column of the chain, whatever the start state
                const unsigned long long keep = __builtin_amdgcn_ballot_w64(kc < Q && !(s < cs * 0x1p-45f));
                const unsigned long long mine = W == 64 ? ~0ull : (((1ull << (W & 63)) - 1ull) << (W * cl));
                risk = risk || (keep & mine) == 0ull;
            }
            cs = s;
            // rescale when any column of the wave has shrunk below 2^-40 (wave-uniform branch; every
            // ~4th step at gene-model emission magnitudes, every ~12th for E ~ 0.5).  0 < cs < 2^-40 as ONE
            // unsigned compare on the bit pattern (cs >= 0; 0 wraps to the top): the ballot is then the compare.
            const unsigned cb = __builtin_bit_cast(unsigned, cs) - 1u;
            if (__builtin_amdgcn_ballot_w64(cb < 0x2B800000u - 1u) != 0) rescale();
        }
    };

    // Q floats of a staged row: whole 16-byte reads plus one 8- / 4-byte read.  Three floats at the end are read
    // with the pad float behind them (HMM_RS_ROW128): the LDS serves a wave's 16-byte read in 4 cycles and its
    // 12-byte read in 8, and with the second-order step the LDS is as busy as the vector unit (the look-ahead copy
    // of a row, HMM_RS_AHEAD, is what the dead fourth register hurt: the allocator hands it out again at once and
    // the prefetch then has to be waited for on the spot).
    auto ldrow = [&](const float *rowp, float (&r)[Q]) {
#pragma unroll
        for (int v = 0; v + 4 <= Q; v += 4) {
            const f4 t = *reinterpret_cast<const f4 *>(rowp + v);
            r[v] = t.x; r[v + 1] = t.y; r[v + 2] = t.z; r[v + 3] = t.w;
        }
        constexpr int R0 = Q & ~3;
        if constexpr (Q - R0 == 3 && HMM_RS_ROW128) {
            static_assert(R0 + 4 <= W, "the pad float belongs to the row");
            const f4 t = *reinterpret_cast<const f4 *>(rowp + R0);
            r[R0] = t.x; r[R0 + 1] = t.y; r[R0 + 2] = t.z;
        } else if constexpr (Q - R0 == 3) {
            typedef float f3 __attribute__((ext_vector_type(3)));
            const f3 t = *reinterpret_cast<const f3 *>(rowp + R0);
            r[R0] = t.x; r[R0 + 1] = t.y; r[R0 + 2] = t.z;
        } else if constexpr (Q - R0 == 2) {
            typedef float f2 __attribute__((ext_vector_type(2)));
            const f2 t = *reinterpret_cast<const f2 *>(rowp + R0);
            r[R0] = t.x; r[R0 + 1] = t.y;
        } else if constexpr (Q - R0 == 1) {
            r[R0] = rowp[R0];
        }
    };

    // The main loop is NOT predicated per lane (a per-lane `if` becomes 15 selects per step):
    // every lane runs to the longest chunk of the wave — rows past a lane's own chunk are
    // finite, clamped emissions of whatever follows — and each lane's result is captured at its
    // own last step.  Only a wave that holds the tail chunk of a sequence (len < T) needs to look
    // for that step as it goes (CHECK, a wave-uniform branch per step); every other wave finishes
    // all its lanes after the last tile.  Each step's emission row is read from LDS one step ahead
    // of its use, so the LDS latency sits under the previous step's ~55 VALU instructions.
    const int ntiles = p.T / SP_TILE;
    const int last = len - 1;                       // -1 for lanes that are not ours
    const bool ragged = __builtin_amdgcn_ballot_w64(mine && len != p.T) != 0;
    auto tile_steps = [&](auto checked, int tile, int buf) {
        constexpr bool CHECK = decltype(checked)::value;
        const float *tp = &ldsw[buf][cl][0];
        // (the 29-state column already fills the register file: no look-ahead copy of the next row there)
        constexpr bool AHEAD = W == 16 && HMM_RS_AHEAD;
        float c[Q], nx[AHEAD ? Q : 1];
        ldrow(tp, c);
        if constexpr (AHEAD) ldrow(tp + W, nx);
        if (tile == 0) {
            // step 0 of a sequence's first chunk has no transition (MsaHmmCell.py:78-79):
            // X = diag(E_0); everyone else takes the generic step
            float xs[Q];
#pragma unroll
            for (int j = 0; j < Q; ++j) xs[j] = O2 ? (j == kc ? 1.f : 0.f) : x[j];
            // (O2: the staged value of a pass-through state carries its incoming weight: the row itself instead)
            float e0 = 1.f;
            if constexpr (O2) { if (first && mine && kc < Q) e0 = fmaxf(E[(chain / p.C) * (long long)p.L * Q + kc], eps); }
            step(pend, c, std::true_type());
            if (first) {
                if constexpr (!O2) e0 = tp[kc < Q ? kc : 0];
#pragma unroll
                for (int j = 0; j < Q; ++j) {                                            // xs = unit column kc
                    x[j] = xs[j] * e0;
                    pend[j] = 1.f;
                    // O2: e0 on a pass-through state is mass in flight, as at a chunk's start but with weight e0
                    if constexpr (O2) { pend[j] = x[j]; xb[j] = flight_src(j) ? 1.f : 0.f; }
                }
                cs = (kc < Q) ? e0 : 0.f;
                ex = 0;
                rescale();
            }
        } else {
            step(pend, c, std::integral_constant<bool, !HMM_RS_SUM2>());
        }
        if (CHECK) { if (__builtin_amdgcn_ballot_w64(tile * SP_TILE == last) != 0) { if (tile * SP_TILE == last) finish(pend); } }
        // steps 1 .. SP_TILE - 1: the odd ones (the tile's last one among them) form the column sum
        auto one = [&](int sidx, auto sumc) {
            if constexpr (AHEAD) {
#pragma unroll
                for (int u = 0; u < Q; ++u) c[u] = nx[u];
                if (sidx + 1 < SP_TILE) ldrow(tp + (sidx + 1) * W, nx);
            } else {
                ldrow(tp + sidx * W, c);
            }
            step(pend, c, sumc);
            if (CHECK) {
                const int t = tile * SP_TILE + sidx;
                if (__builtin_amdgcn_ballot_w64(t == last) != 0) { if (t == last) finish(pend); }
            }
        };
#pragma unroll
        for (int sidx = 1; sidx < SP_TILE; sidx += 2) {
            one(sidx, std::true_type());
            if (sidx + 1 < SP_TILE) one(sidx + 1, std::integral_constant<bool, !HMM_RS_SUM2>());
        }
    };
    // QR: the same tile with the row in the quad.  Step s reads its row into rq[s & 1] and takes the pass-through
    // weights from rq[(s & 1) ^ 1], the row of the step before; SP_TILE is even, so a tile's last row waits in rq[1]
    // for the next tile's step 0.  The two sets are written by the LDS reads alone (no copy: see quad_mul).
    // A chunk's first two steps run in the per-lane form on whole rows: a column that starts on a pass-through state
    // is a unit of mass in flight that one lane alone sees in front of step 0 (and, on a sequence's first chunk, with
    // weight e0 in front of step 1), which no staged row can express.  For every other lane the per-lane weights of
    // step 1 are row 0's values, the numbers the quad would hold.
    auto tile_steps_quad = [&](auto checked, int tile, int buf) {
        constexpr bool CHECK = decltype(checked)::value;
        static_assert(SP_TILE % 2 == 0 && SP_TILE >= 4, "two row sets, rotated by the step pair");
        const float *tp = &ldsw[buf][cl][0];
        const float *qp = tp + 4 * (kc & 3);             // (the pad lane: floats 12-15, as lane 11)
        auto ldquad = [&](int sidx) { return *reinterpret_cast<const f4 *>(qp + sidx * W); };
        auto done = [&](int sidx, const auto &pw) {
            if (CHECK) {
                const int t = tile * SP_TILE + sidx;
                if (__builtin_amdgcn_ballot_w64(t == last) != 0) { if (t == last) finish(pw); }
            }
        };
        if (tile == 0) {
            float c[Q], pl[Q];
#pragma unroll
            for (int j = 0; j < Q; ++j) {                // the unit column kc, in flight if kc is a pass-through state
                pl[j] = (j == kc) ? 1.f : 0.f;
                if (live(j)) { x[j] = pl[j]; xb[j] = flight_src(j) ? 1.f : 0.f; }
            }
            ldrow(tp, c);
            float e0 = 1.f;
            if (first && mine && kc < Q) e0 = fmaxf(E[(chain / p.C) * (long long)p.L * Q + kc], eps);
            step(pl, c, std::true_type());
            if (first) {           // step 0 of a sequence's first chunk has no transition: X = diag(E_0), see tile_steps
#pragma unroll
                for (int j = 0; j < Q; ++j) {
                    x[j] = ((j == kc) ? 1.f : 0.f) * e0;
                    pl[j] = x[j];
                    xb[j] = flight_src(j) ? 1.f : 0.f;
                }
                cs = (kc < Q) ? e0 : 0.f;
                ex = 0;
                rescale();
            }
            done(0, pl);
            ldrow(tp + W, c);
            step(pl, c, std::true_type());
            done(1, pl);
            rq[1] = ldquad(1);
        } else {
            rq[0] = ldquad(0);
            step(rq[1], rq[0], std::integral_constant<bool, !HMM_RS_SUM2>());
            done(0, rq[0]);
            rq[1] = ldquad(1);
            step(rq[0], rq[1], std::true_type());
            done(1, rq[1]);
        }
        // steps 2 .. SP_TILE - 1: the odd ones (the tile's last one among them) form the column sum, or its gate
#pragma unroll
        for (int sidx = 2; sidx < SP_TILE; sidx += 2) {
            rq[0] = ldquad(sidx);
            step(rq[1], rq[0], std::integral_constant<bool, !HMM_RS_SUM2>());
            done(sidx, rq[0]);
            rq[1] = ldquad(sidx + 1);
            step(rq[0], rq[1], std::true_type());
            done(sidx + 1, rq[1]);
        }
    };
    auto run_tile = [&](auto checked, int tile) {
        if constexpr (QR) tile_steps_quad(checked, tile, tile & 1);
        else tile_steps(checked, tile, tile & 1);
    };
    fetch(0);
    if (ragged) {
        for (int tile = 0; tile < ntiles; ++tile) {
            stage(tile & 1);
            if (tile + 1 < ntiles) fetch(tile + 1);
            run_tile(std::true_type(), tile);
        }
    } else {
        for (int tile = 0; tile < ntiles; ++tile) {
            stage(tile & 1);
            if (tile + 1 < ntiles) fetch(tile + 1);
            run_tile(std::false_type(), tile);
        }
        if (mine) {
            if constexpr (QR) finish(rq[1]);
            else finish(pend);
        }
    }
}

// MIXED: the launch for waves that straddle two models (k > 1 only); every other wave belongs to the main launch
template <class T, bool MIXED>
__device__ __forceinline__ void reduce_sparse_block(const float *__restrict__ A, const float *__restrict__ E,
                                                    float *__restrict__ ops, int *__restrict__ exps,
                                                    const int *__restrict__ topo, const Plan &p, float eps) {
    // [wave][buffer][chain in wave][step][16 floats: one clamped emission row, 64-byte stride]
    // chain images are 1 KB; +16 floats of padding puts the 4 chains of a wave on different banks
    __shared__ __attribute__((aligned(16))) typename RsCfg<T>::Lds lds[4];
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63, cl = lane / RsCfg<T>::W;
    const long long wchain0 = ((long long)blockIdx.x * 4 + w) * RsCfg<T>::CPW;          // first chain of the wave
    if (wchain0 >= p.nchains) return;
    const long long chain = wchain0 + cl;
    const bool inrange = chain < p.nchains;
    const long long chn = inrange ? chain : wchain0;
    const int seq = (int)(chn / p.C), c = (int)(chn - (long long)seq * p.C);
    const int m = seq / p.b;
    const int tp = topo[m];
    const bool mine = inrange && (tp & (TOPO_UNIT - 1)) == T::ID && tp != TOPO_EXACT;
    // wave-uniform early out when none of the four chains is ours
    const unsigned long long mmask = __builtin_amdgcn_ballot_w64(mine);
    if (mmask == 0) return;
    // the unit-weight variant when every chain of the wave that is ours qualifies (models can mix in a wave)
    const bool unit = __builtin_amdgcn_ballot_w64(mine && (tp & TOPO_UNIT)) == mmask;
    const bool uni = HMM_RS_UNI && __builtin_amdgcn_ballot_w64(m != __builtin_amdgcn_readfirstlane(m)) == 0ull;
    if (uni == MIXED) return;                    // the other launch has this wave
    if (unit) reduce_sparse_wave<T, true, !MIXED>(A, E, ops, exps, p, eps, lds[w], wchain0, mine, m, chain, c);
    else reduce_sparse_wave<T, false, !MIXED>(A, E, ops, exps, p, eps, lds[w], wchain0, mine, m, chain, c);
}

// 16 lanes per chain (7 / 15 states): held to HMM_RS_WPE waves per SIMD
template <class T, bool MIXED = false>
__global__ __launch_bounds__(256) RS_ATTR void k_reduce_sparse(const float *__restrict__ A, const float *__restrict__ E,
                                                       float *__restrict__ ops, int *__restrict__ exps,
                                                       const int *__restrict__ topo, Plan p, float eps) {
    reduce_sparse_block<T, MIXED>(A, E, ops, exps, topo, p, eps);
}
// 32 lanes per chain (29 states): the column alone takes ~230 registers, two waves per SIMD
template <class T, bool MIXED = false>
__global__ __launch_bounds__(256) void k_reduce_sparse_wide(const float *__restrict__ A, const float *__restrict__ E,
                                                            float *__restrict__ ops, int *__restrict__ exps,
                                                            const int *__restrict__ topo, Plan p, float eps) {
    reduce_sparse_block<T, MIXED>(A, E, ops, exps, topo, p, eps);
}

// ------------------------------------------------------------------ scan

// 16-lane (DPP row) all-reduce and lane broadcast without LDS: ds_bpermute shuffles made every
// hop of the scan ~1.6 us of pure latency (24 dependent shuffles); these are plain VALU ops.
template <class Op>
__device__ __forceinline__ int row_allreduce_i(int v, Op op) {
    v = op(v, __builtin_amdgcn_update_dpp(v, v, 0xB1, 0xF, 0xF, false));    // quad_perm [1,0,3,2]
    v = op(v, __builtin_amdgcn_update_dpp(v, v, 0x4E, 0xF, 0xF, false));    // quad_perm [2,3,0,1]
    v = op(v, __builtin_amdgcn_update_dpp(v, v, 0x141, 0xF, 0xF, false));   // row_half_mirror
    v = op(v, __builtin_amdgcn_update_dpp(v, v, 0x140, 0xF, 0xF, false));   // row_mirror
    return v;
}
__device__ __forceinline__ float row_sum_f(float x) {
    int v = __builtin_bit_cast(int, x);
    auto add = [](int a, int b) { return __builtin_bit_cast(int, __builtin_bit_cast(float, a) + __builtin_bit_cast(float, b)); };
    return __builtin_bit_cast(float, row_allreduce_i(v, add));
}
__device__ __forceinline__ int row_max_i(int x) {
    return row_allreduce_i(x, [](int a, int b) { return a > b ? a : b; });
}
__device__ __forceinline__ float lane_bcast(float x, int srclane) {      // srclane wave-uniform
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), srclane));
}
// lane K of this lane's 16-lane row, in every lane of the row (DPP row_newbcast): four independent
// 16-lane problems per wave
template <int K>
__device__ __forceinline__ float row_bcast_f(float x) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x150 + K, 0xF, 0xF, false));
}
// sum_k c[k] * (lane k of v's row)
__device__ __forceinline__ float row_dot16(const float (&c)[16], float v) {
    float a0 = 0.f, a1 = 0.f;
    a0 = fmaf(c[0], row_bcast_f<0>(v), a0);   a1 = fmaf(c[1], row_bcast_f<1>(v), a1);
    a0 = fmaf(c[2], row_bcast_f<2>(v), a0);   a1 = fmaf(c[3], row_bcast_f<3>(v), a1);
    a0 = fmaf(c[4], row_bcast_f<4>(v), a0);   a1 = fmaf(c[5], row_bcast_f<5>(v), a1);
    a0 = fmaf(c[6], row_bcast_f<6>(v), a0);   a1 = fmaf(c[7], row_bcast_f<7>(v), a1);
    a0 = fmaf(c[8], row_bcast_f<8>(v), a0);   a1 = fmaf(c[9], row_bcast_f<9>(v), a1);
    a0 = fmaf(c[10], row_bcast_f<10>(v), a0); a1 = fmaf(c[11], row_bcast_f<11>(v), a1);
    a0 = fmaf(c[12], row_bcast_f<12>(v), a0); a1 = fmaf(c[13], row_bcast_f<13>(v), a1);
    a0 = fmaf(c[14], row_bcast_f<14>(v), a0); a1 = fmaf(c[15], row_bcast_f<15>(v), a1);
    return a0 + a1;
}

// One 128-thread block per sequence: wave 0 runs the forward prefix chain, wave 1 the backward
// suffix chain (separate waves so the two dependent chains run concurrently), 16 lanes each.
// C hops per chain, every hop a 16x16 mat-vec.
__global__ __launch_bounds__(128) void k_scan(const float *__restrict__ pi, const float *__restrict__ ops,
                                             const int *__restrict__ exps, float *__restrict__ prefix,
                                             double *__restrict__ llpre, float *__restrict__ suffix,
                                             double *__restrict__ lsuf, double *__restrict__ loglik,
                                             const int *__restrict__ topo, Plan p, float eps,
                                             const float *__restrict__ pre_in = nullptr,
                                             const double *__restrict__ ll_in = nullptr,
                                             const float *__restrict__ suf_in = nullptr,
                                             const double *__restrict__ ls_in = nullptr) {
    // pre_in / ll_in / suf_in / ls_in (sequence-sharded calls): the vectors entering this time slab
    // from the slabs before / after it, in place of the start distribution and of ones
    const int seq = blockIdx.x;
    const int lane = threadIdx.x & 63;
    const int dir = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int n = lane & 15;
    const int q = p.q, C = p.C;
    const int m = seq / p.b;
    const size_t chain0 = (size_t)seq * C;
    if (lane >= 16) return;
    if (topo[m] == TOPO_EXACT) return;          // served by the serial exact-clamp kernels
    if (dir == 0) {
        float praw = pre_in ? pre_in[(size_t)seq * QP + n] : ((n < q) ? pi[(size_t)m * q + n] : 0.f);
        float a = pre_in ? praw : ((n < q) ? fmaxf(praw, eps) : 0.f);
        double ll = ll_in ? ll_in[seq] : 0.0;
        prefix[chain0 * QP + n] = praw;
        if (n == 0) llpre[chain0] = ll;
        // operator rows are prefetched one hop ahead: the hop itself is ~100 cycles of math, a
        // dependent 1 KB load per hop would make the scan a chain of C memory round trips
        const f4 *row = reinterpret_cast<const f4 *>(ops + chain0 * QP * QP + n * QP);
        f4 r0 = row[0], r1 = row[1], r2 = row[2], r3 = row[3];
        int xe = exps[chain0 * QP + n];
        for (int c = 0; c < C; ++c) {
            const f4 q0 = r0, q1 = r1, q2 = r2, q3 = r3;
            const int xec = xe;
            if (c + 1 < C) {
                const f4 *nx = reinterpret_cast<const f4 *>(ops + (chain0 + c + 1) * QP * QP + n * QP);
                r0 = nx[0]; r1 = nx[1]; r2 = nx[2]; r3 = nx[3];
                xe = exps[(chain0 + c + 1) * QP + n];
            }
            int we = (a > 0.f) ? __builtin_amdgcn_frexp_expf(a) + xec : -(1 << 28);
            const int emax = row_max_i(we);
            int sh = xec - emax;
            sh = sh < -300 ? -300 : sh;
            float w = __builtin_amdgcn_ldexpf(a, sh);
            float acc = 0.f;
            float xr[16] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, q3.x, q3.y, q3.z, q3.w};
#pragma unroll
            for (int kk = 0; kk < 16; ++kk) acc = fmaf(xr[kk], lane_bcast(w, kk), acc);
            const float S = row_sum_f(acc);
            a = acc / S;
            ll += (double)__logf(S) + (double)emax * LN2;
            if (c + 1 < C) {
                prefix[(chain0 + c + 1) * QP + n] = a;
                if (n == 0) llpre[chain0 + c + 1] = ll;
            }
        }
        if (n == 0) loglik[seq] = ll;
    } else {
        float v = suf_in ? suf_in[(size_t)seq * QP + n] : ((n < q) ? 1.f : 0.f);
        double lb = ls_in ? ls_in[seq] : 0.0;
        // column n of the operator (stride QP), prefetched one hop ahead like the forward chain
        float col[16];
        int xe = 0;
        if (C > 1) {
            const float *X = ops + (chain0 + C - 1) * QP * QP;
#pragma unroll
            for (int j = 0; j < 16; ++j) col[j] = X[j * QP + n];
            xe = exps[(chain0 + C - 1) * QP + n];
        }
        for (int c = C - 1; c >= 0; --c) {
            suffix[(chain0 + c) * QP + n] = v;
            if (n == 0) lsuf[chain0 + c] = lb;
            if (c == 0) break;
            float cc[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) cc[j] = col[j];
            const int xec = xe;
            if (c - 1 > 0) {
                const float *X = ops + (chain0 + c - 1) * QP * QP;
#pragma unroll
                for (int j = 0; j < 16; ++j) col[j] = X[j * QP + n];
                xe = exps[(chain0 + c - 1) * QP + n];
            }
            float u = 0.f;
#pragma unroll
            for (int j = 0; j < 16; ++j) u = fmaf(cc[j], lane_bcast(v, j), u);
            int we = (u > 0.f) ? __builtin_amdgcn_frexp_expf(u) + xec : -(1 << 28);
            const int emax = row_max_i(we);
            int sh = xec - emax;
            sh = sh < -300 ? -300 : sh;
            v = __builtin_amdgcn_ldexpf(u, sh);
            lb += (double)emax * LN2;
        }
    }
}

// ---- two-level chunk scan.  The hops above are linear (no clamps at this level), so operators
// compose exactly up to rounding: groups of ~sqrt(C) chunks are composed in parallel
// (k_scan_compose), k_scan itself runs over the G group operators, and k_scan_inner walks the
// chunks of every group in parallel from the group's entry vectors.  Serial depth ~3 sqrt(C) hops
// instead of C (196 -> 42 at b = 1024 x L = 1e5; 1954 -> 135 for one sequence of 1e6).
__device__ __forceinline__ int col_max_i(int v) {       // max over the four lanes of a tile column
    float a = __builtin_bit_cast(float, v), b2 = a;
    swap16(a, b2);
    v = max(__builtin_bit_cast(int, a), __builtin_bit_cast(int, b2));
    a = __builtin_bit_cast(float, v); b2 = a;
    swap32(a, b2);
    return max(__builtin_bit_cast(int, a), __builtin_bit_cast(int, b2));
}

// one wave per (sequence, group): X <- Op_c X over the group's chunks, X = identity at the start.
// Tile layout of k_reduce: lane (g, n) holds rows 4g..4g+3 of column n, column n scaled by 2^-ex.
__global__ __launch_bounds__(256) void k_scan_compose(const float *__restrict__ ops, const int *__restrict__ exps,
                                                      float *__restrict__ gops, int *__restrict__ gexps,
                                                      const int *__restrict__ topo, Plan p) {
    const long long wv = (long long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (wv >= (long long)p.NB * p.G) return;
    const int lane = threadIdx.x & 63, g = lane >> 4, n = lane & 15;
    const int seq = (int)(wv / p.G), grp = (int)(wv - (long long)seq * p.G);
    if (topo[seq / p.b] == TOPO_EXACT) return;
    const int c0 = grp * p.gsize, c1 = min(p.C, c0 + p.gsize);
    f4 X = {4 * g + 0 == n ? 1.f : 0.f, 4 * g + 1 == n ? 1.f : 0.f, 4 * g + 2 == n ? 1.f : 0.f, 4 * g + 3 == n ? 1.f : 0.f};
    int ex = 0;
    // A-operand: lane (g, i = n) supplies Op_c[i][4g + kk]; exponents of the contraction rows 4g + r.
    // The operands of the next SCAN_PF hops are in flight during this one.
    const size_t chb = (size_t)seq * p.C;
    f4 an[SCAN_PF];
    i4 en[SCAN_PF];
#pragma unroll
    for (int u = 0; u < SCAN_PF; ++u) {
        const int c = min(c0 + u, c1 - 1);
        an[u] = *reinterpret_cast<const f4 *>(ops + (chb + c) * QP * QP + n * QP + 4 * g);
        en[u] = *reinterpret_cast<const i4 *>(exps + (chb + c) * QP + 4 * g);
    }
    for (int cb = c0; cb < c1; cb += SCAN_PF)
#pragma unroll
      for (int u = 0; u < SCAN_PF; ++u) {
        const int c = cb + u;
        if (c >= c1) break;                                   // wave-uniform
        const f4 a4 = an[u];
        const i4 e4 = en[u];
        if (c + SCAN_PF < c1) {
            an[u] = *reinterpret_cast<const f4 *>(ops + (chb + c + SCAN_PF) * QP * QP + n * QP + 4 * g);
            en[u] = *reinterpret_cast<const i4 *>(exps + (chb + c + SCAN_PF) * QP + 4 * g);
        }
        // align the rows of X to a common exponent per column
        int we = -(1 << 28);
        we = X.x > 0.f ? max(we, __builtin_amdgcn_frexp_expf(X.x) + e4.x) : we;
        we = X.y > 0.f ? max(we, __builtin_amdgcn_frexp_expf(X.y) + e4.y) : we;
        we = X.z > 0.f ? max(we, __builtin_amdgcn_frexp_expf(X.z) + e4.z) : we;
        we = X.w > 0.f ? max(we, __builtin_amdgcn_frexp_expf(X.w) + e4.w) : we;
        const int emax = col_max_i(we);
        f4 W;
        W.x = __builtin_amdgcn_ldexpf(X.x, max(e4.x - emax, -300));
        W.y = __builtin_amdgcn_ldexpf(X.y, max(e4.y - emax, -300));
        W.z = __builtin_amdgcn_ldexpf(X.z, max(e4.z - emax, -300));
        W.w = __builtin_amdgcn_ldexpf(X.w, max(e4.w - emax, -300));
        const float af[4] = {a4.x, a4.y, a4.z, a4.w};
        X = mfma4(af, W);
        // bring the column sum back into [0.5, 1): exact power of two
        const float sden = col_sum(hsum(X));
        const int xe = __builtin_amdgcn_frexp_expf(sden);
        X = X * __builtin_amdgcn_ldexpf(1.0f, -xe);
        ex += emax + xe;
    }
    float *o = gops + (size_t)wv * QP * QP;
    o[(4 * g + 0) * QP + n] = X.x;
    o[(4 * g + 1) * QP + n] = X.y;
    o[(4 * g + 2) * QP + n] = X.z;
    o[(4 * g + 3) * QP + n] = X.w;
    if (g == 0) gexps[(size_t)wv * QP + n] = ex;
}

// one block per (sequence, group): the hops of k_scan over the group's chunks, started from the
// group's entry vectors (gprefix / gllpre forward, gsuffix / glsuf backward) that k_scan left.
__global__ __launch_bounds__(128) void k_scan_inner(const float *__restrict__ ops, const int *__restrict__ exps,
                                                   const float *__restrict__ gprefix, const double *__restrict__ gllpre,
                                                   const float *__restrict__ gsuffix, const double *__restrict__ glsuf,
                                                   float *__restrict__ prefix, double *__restrict__ llpre,
                                                   float *__restrict__ suffix, double *__restrict__ lsuf,
                                                   const int *__restrict__ topo, Plan p, float eps) {
    // wave 0 of the block: forward prefixes, wave 1: backward suffixes; a 16-lane row per (sequence, group),
    // FOUR of them per wave (row sums / maxima and the row broadcast are DPP operations inside the row), the
    // loops run to the longest row's count
    const int lane = threadIdx.x & 63;
    const int dir = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int n = lane & 15;
    const int q = p.q;
    const long long blk = (long long)blockIdx.x * 4 + (lane >> 4);
    bool valid = blk < (long long)p.NB * p.G;
    const long long bl = valid ? blk : 0;
    const int seq = (int)(bl / p.G), grp = (int)(bl - (long long)seq * p.G);
    valid = valid && topo[seq / p.b] != TOPO_EXACT;
    const int c0 = grp * p.gsize, c1 = min(p.C, c0 + p.gsize);
    const size_t chain0 = (size_t)seq * p.C;
    int hops = valid ? c1 - 1 - c0 : 0;
    for (int o = 32; o > 0; o >>= 1) hops = max(hops, __shfl_xor(hops, o));
    if (dir == 0) {
        const float pin = valid ? gprefix[(size_t)bl * QP + n] : 0.f;
        // the sequence's very first vector is the raw start distribution: clamped for the recursion,
        // stored raw (the apply kernel clamps it itself), as in k_scan
        float a = (grp == 0 && p.seq_start) ? ((n < q) ? fmaxf(pin, eps) : 0.f) : pin;
        double ll = valid ? gllpre[bl] : 0.0;
        if (valid) {
            prefix[(chain0 + c0) * QP + n] = pin;
            if (n == 0) llpre[chain0 + c0] = ll;
        }
        float rw[SCAN_PF][16];
        int xe[SCAN_PF];
        auto fetch = [&](int u, int c) {                      // row n of operator c, exponent of source state n -> slot u
            const f4 *row = reinterpret_cast<const f4 *>(ops + (chain0 + c) * QP * QP + n * QP);
            const f4 r0 = row[0], r1 = row[1], r2 = row[2], r3 = row[3];
            rw[u][0] = r0.x; rw[u][1] = r0.y; rw[u][2] = r0.z; rw[u][3] = r0.w; rw[u][4] = r1.x; rw[u][5] = r1.y;
            rw[u][6] = r1.z; rw[u][7] = r1.w; rw[u][8] = r2.x; rw[u][9] = r2.y; rw[u][10] = r2.z; rw[u][11] = r2.w;
            rw[u][12] = r3.x; rw[u][13] = r3.y; rw[u][14] = r3.z; rw[u][15] = r3.w;
            xe[u] = exps[(chain0 + c) * QP + n];
        };
#pragma unroll
        for (int u = 0; u < SCAN_PF; ++u) {
            xe[u] = 0;
#pragma unroll
            for (int k = 0; k < 16; ++k) rw[u][k] = 0.f;
            if (valid && c0 + u + 1 < c1) fetch(u, c0 + u);
        }
        for (int hb = 0; hb < hops; hb += SCAN_PF)
#pragma unroll
          for (int u = 0; u < SCAN_PF; ++u) {
            const int h = hb + u;
            if (h >= hops) break;                             // wave-uniform
            const int c = c0 + h;
            const bool on = valid && c + 1 < c1;
            float cur[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) cur[k] = rw[u][k];
            const int xec = xe[u];
            if (valid && c + SCAN_PF + 1 < c1) fetch(u, c + SCAN_PF);
            int we = (a > 0.f) ? __builtin_amdgcn_frexp_expf(a) + xec : -(1 << 28);
            const int emax = row_max_i(we);
            int sh = xec - emax;
            sh = sh < -300 ? -300 : sh;
            const float w = __builtin_amdgcn_ldexpf(a, sh);
            const float acc = row_dot16(cur, w);
            const float S = row_sum_f(acc);
            if (on) {
                a = acc / S;
                ll += (double)__logf(S) + (double)emax * LN2;
                prefix[(chain0 + c + 1) * QP + n] = a;
                if (n == 0) llpre[chain0 + c + 1] = ll;
            }
        }
    } else {
        float v = valid ? gsuffix[(size_t)bl * QP + n] : 0.f;
        double lb = valid ? glsuf[bl] : 0.0;
        float col[SCAN_PF][16];
        int xe[SCAN_PF];
        auto fetch = [&](int u, int c) {                      // column n of operator c -> slot u
            const float *X = ops + (chain0 + c) * QP * QP;
#pragma unroll
            for (int j = 0; j < 16; ++j) col[u][j] = X[j * QP + n];
            xe[u] = exps[(chain0 + c) * QP + n];
        };
        if (valid) {
            suffix[(chain0 + c1 - 1) * QP + n] = v;
            if (n == 0) lsuf[chain0 + c1 - 1] = lb;
        }
#pragma unroll
        for (int u = 0; u < SCAN_PF; ++u) {
            xe[u] = 0;
#pragma unroll
            for (int j = 0; j < 16; ++j) col[u][j] = 0.f;
            if (valid && c1 - 1 - u > c0) fetch(u, c1 - 1 - u);
        }
        for (int hb = 0; hb < hops; hb += SCAN_PF)
#pragma unroll
          for (int u = 0; u < SCAN_PF; ++u) {
            const int h = hb + u;
            if (h >= hops) break;                             // wave-uniform
            const int c = c1 - 1 - h;                         // through operator c: the suffix of chunk c - 1
            const bool on = valid && c > c0;
            float cc[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) cc[j] = col[u][j];
            const int xec = xe[u];
            if (valid && c - SCAN_PF > c0) fetch(u, c - SCAN_PF);
            const float un = row_dot16(cc, v);
            int we = (un > 0.f) ? __builtin_amdgcn_frexp_expf(un) + xec : -(1 << 28);
            const int emax = row_max_i(we);
            int sh = xec - emax;
            sh = sh < -300 ? -300 : sh;
            if (on) {
                v = __builtin_amdgcn_ldexpf(un, sh);
                lb += (double)emax * LN2;
                suffix[(chain0 + c - 1) * QP + n] = v;
                if (n == 0) lsuf[chain0 + c - 1] = lb;
            }
        }
    }
}

// ------------------------------------------------------------------ apply (shared pieces)

struct Tile {                 // what one wave of an apply kernel works on: 16 chains
    long long wave;           // index of the wave in its plan
    long long chain;          // this lane's chain (column n)
    bool valid;
    bool first;               // chunk 0 of its sequence
    int len;                  // steps in this chain's chunk (0 if !valid)
    int voff;                 // byte offset of element (t0, 4g) relative to the wave base
    __amdgpu_buffer_rsrc_t rsE;
    const float *baseE;       // wave base pointer (for the matching output base)
};

__device__ __forceinline__ Tile make_tile(const float *E, const Plan &p, long long wave, int g, int n,
                                          int *model, long long *wchain0) {
    // waves never straddle models: each model owns ceil(b*C/16) waves
    const long long per_model = (long long)p.b * p.C;
    const long long wpm = (per_model + p.cpw - 1) / p.cpw;
    const int m = (int)(wave / wpm);
    const long long w = wave - (long long)m * wpm;
    const long long c0 = (long long)m * per_model + w * p.cpw;       // first chain of the wave
    Tile tl;
    tl.wave = wave;
    long long rel = w * p.cpw + n;
    tl.valid = n < p.cpw && rel < per_model;
    tl.chain = c0 + (tl.valid ? n : 0);
    const long long seq = tl.chain / p.C;
    const int c = (int)(tl.chain - seq * p.C);
    const long long seq0 = c0 / p.C;
    const int cc0 = (int)(c0 - seq0 * p.C);
    tl.first = (c == 0) && p.seq_start;
    tl.len = tl.valid ? min(p.T, p.L - c * p.T) : 0;
    const long long row0 = seq0 * p.L + (long long)cc0 * p.T;        // wave base row
    const long long row = seq * p.L + (long long)c * p.T;
    tl.voff = (int)((row - row0) * p.q * (long long)sizeof(float)) + g * 16;
    const unsigned long long total = (unsigned long long)p.NB * p.L * p.q * sizeof(float);
    const unsigned long long boff = (unsigned long long)row0 * p.q * sizeof(float);
    tl.baseE = E + row0 * p.q;
    tl.rsE = make_rsrc(tl.baseE, total - boff);
    *model = m;
    *wchain0 = c0;
    return tl;
}

// ---- output staging.  A wave produces, per step, 16 rows (one per chain) of q floats spread
// over its lanes as 16-byte pieces; storing those directly touches 16 different cache lines
// with 16/12-byte fragments per instruction and made the posterior kernel store-bound
// (3.9 ms with, 2.1 ms without its stores).  Instead the rows are collected in wave-private LDS —
// per chain one contiguous run of rows, exactly its image in HBM — and flushed as full 16-byte
// pieces of contiguous memory, OUT_ROWS rows of every chain at a time.  The size of those bursts
// is what the HBM system rewards in a read + write stream (tools/experiments/stream_pattern.hip, the
// kernels' own access pattern with no arithmetic: 480-byte visits per chain 3.97 TB/s, 960-byte
// 4.74, 1920-byte 5.11); 32 rows of 60 bytes are also exactly 15 cache lines, so the groups of a
// line-aligned chunk share no line with their neighbours.
#ifndef HMM_OUT_ROWS
#define HMM_OUT_ROWS 16                                // rows per chain staged in LDS per flush (multiple of SUB)
#endif
#define OUT_GB (HMM_OUT_ROWS / SUB)                    // apply blocks per flush group
#define OUT_STRIDE (HMM_OUT_ROWS * QP + 4)             // floats per chain in LDS (16-byte multiple)
#define OUT_SEG (16 * OUT_STRIDE + 32)                 // floats per wave: the staged rows + the chain table

typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));
struct __attribute__((packed, aligned(4))) P4 { float a, b, c, d; };
struct __attribute__((packed, aligned(4))) P3 { float a, b, c; };
struct __attribute__((packed, aligned(4))) P2 { float a, b; };

struct OutStage {
    float *seg;                 // this wave's LDS region: 16 chains x OUT_STRIDE floats, then the chain table
    char *base;                 // global base pointer of the wave (same origin as the E descriptor)
    int q;
};

// chain table at the end of the segment: [c] byte offset of chain c's chunk start, [16 + c] its valid steps
__device__ __forceinline__ OutStage make_outstage(float *seg, char *base, int q, int lane, int voff0, int len) {
    OutStage o;
    o.seg = seg; o.base = base; o.q = q;
    int *tab = reinterpret_cast<int *>(seg + 16 * OUT_STRIDE);
    if (lane < 16) { tab[lane] = voff0; tab[16 + lane] = len; }        // lane c (g = 0) owns chain c
    __builtin_amdgcn_wave_barrier();
    return o;
}

// put states 4g..4g+3 of chain n's row `s` (relative to the flush group) into the stage
__device__ __forceinline__ void stage_row(const OutStage &o, int n, int g, int s, f4 v) {
    float *p = o.seg + n * OUT_STRIDE + s * o.q + 4 * g;
    const int nv = o.q - 4 * g;
#if HMM_STAGE_BF
    // Four unconditional writes, for every q and both walking directions: a component that is not in the row
    // (state 4g + i >= q; all four where the lane's window lies outside the row) goes to float i of the chain's
    // 4-float pad at the end of its OUT_STRIDE instead — nothing reads the pad (flush_rows and decode_rows stop
    // below HMM_OUT_ROWS * q <= HMM_OUT_ROWS * QP floats, permute_rows' blocks end there too).  The predicates are
    // the lane's own for the whole kernel, so a write costs one select on its address and no exec-mask region.
    float *d = o.seg + n * OUT_STRIDE + HMM_OUT_ROWS * QP;
    (nv >= 1 ? p : d)[0] = v.x;
    (nv >= 2 ? p : d)[1] = v.y;
    (nv >= 3 ? p : d)[2] = v.z;
    (nv >= 4 ? p : d)[3] = v.w;
#else
    if (nv >= 1) p[0] = v.x;
    if (nv >= 2) p[1] = v.y;
    if (nv >= 3) p[2] = v.z;
    if (nv >= 4) p[3] = v.w;
#endif
}

// write the staged rows row0 .. row0+nrows-1 (chunk-relative; nrows a multiple of 4, at most
// OUT_ROWS) of every chain to global memory: consecutive lanes take consecutive 16-byte pieces
__device__ __forceinline__ void flush_rows(const OutStage &o, int lane, int row0, int nrows) {
    const int ppc = nrows * o.q / 4;                                   // pieces per chain
    const float inv = 1.0f / (float)ppc;
    const int *tab = reinterpret_cast<const int *>(o.seg + 16 * OUT_STRIDE);
    __builtin_amdgcn_wave_barrier();
    for (int pc = lane; pc < 16 * ppc; pc += 64) {
        const int c = (int)(((float)pc + 0.5f) * inv);                 // pc / ppc, exact for these ranges
        const int kk = pc - c * ppc;
        int rows = tab[16 + c] - row0;
        rows = rows > nrows ? nrows : rows;
        const int nfl = rows * o.q - 4 * kk;                           // floats of this piece that exist
        if (nfl <= 0) continue;
        const f4 v = *reinterpret_cast<const f4 *>(o.seg + c * OUT_STRIDE + 4 * kk);
        char *dst = o.base + tab[c] + (row0 * o.q + 4 * kk) * (int)sizeof(float);
#if HMM_NT_STORE
        // the output is never read back by these kernels: streaming stores leave L2 to the emission rows and
        // checkpoints (k_backward 2.97 -> 2.86 ms; the same hint on the emission LOADS costs 20-45 %)
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

// ---- decoded output (hmm_posterior_decode): the output policy of backward_body.  NoDecode writes the staged rows
// themselves (flush_rows); Decode collapses every staged gamma row to (class with the largest posterior, that
// posterior) and writes 1 + 4 bytes per position instead of 4 q.  The rows are staged exactly as for the full
// output — the same values in the same LDS segment — and lane i of a flush takes row i % nrows of chain i / nrows:
// it reads the row's q floats back (rows are q floats apart, so the lanes of an odd q are on distinct banks), sums
// the states of every class in increasing state index, and stores one byte and one float.  Consecutive lanes hold
// consecutive positions of a chain, so a store instruction writes runs of nrows label bytes / nrows floats per chain;
// every lane addresses its own byte, so a chunk that starts at any byte offset and a ragged last group need nothing
// special.  The class table travels in the kernel arguments as a 0 / 1 weight per (class, state): a class sum is one
// scalar load of the class's 16 weights and 16 fused multiply-adds with a scalar operand (fma(v, 1, sum) is sum + v
// rounded once, fma(v, 0, sum) is sum), with no per-state test anywhere — testing a packed table on the scalar unit
// cost four scalar instructions per (class, state) and more time than the smaller output saved.
struct NoDecode {
    static constexpr bool on = false;
};
struct alignas(64) Decode {
    static constexpr bool on = true;
    float w[QP][QP];             // w[c][s] = 1 where state s belongs to class c, else 0
    unsigned char *label;        // (k,b,L)
    float *conf;                 // (k,b,L) or null
    int ncls;                    // number of classes; 0: the identity map (no sums)
    void advance(size_t rows) { label += rows; if (conf) conf += rows; }      // host: a batch group's first row
};
// ClassOut (hmm_class_posterior): Decode without the argmax — the same staging, weight table and class-sum loop, so
// the sums have the bits Decode compares — and every class's sum is stored: (k,b,L,ncls) floats to `prob` and / or
// `logp`, where an elementwise kernel turns them into their logs after the pass (hmm_class_posterior.inc).
struct alignas(64) ClassOut {
    static constexpr bool on = true;
    float w[QP][QP];             // w[c][s] = 1 where state s belongs to class c, else 0
    float *prob;                 // (k,b,L,ncls) or null
    float *logp;                 // (k,b,L,ncls) or null: receives the sums as well
    int ncls;                    // 1..QP
    void advance(size_t rows) { if (prob) prob += rows * ncls; if (logp) logp += rows * ncls; }
};

// Decode's flush: the chain table holds ROW offsets from `rowbase` (the wave's first row in the (k,b,L) outputs)
__device__ __forceinline__ void decode_rows(const OutStage &o, const Decode &d, long long rowbase, int lane, int row0,
                                            int nrows) {
    const float inv = 1.0f / (float)nrows;
    const int *tab = reinterpret_cast<const int *>(o.seg + 16 * OUT_STRIDE);
    __builtin_amdgcn_wave_barrier();
#pragma unroll 1                                                       // (one row's values in registers at a time)
    for (int pc = lane; pc < 16 * nrows; pc += 64) {
        const int c = (int)(((float)pc + 0.5f) * inv);                 // pc / nrows, exact for these ranges
        const int r = pc - c * nrows;
        if (r >= tab[16 + c] - row0) continue;                         // (a chain's ragged end; chains the wave does not own)
        const float *row = o.seg + c * OUT_STRIDE + r * o.q;
        float v[QP];
#pragma unroll
        for (int s = 0; s < QP; ++s) v[s] = s < o.q ? row[s] : 0.f;
        float best = v[0];
        int lab = 0;
        if (d.ncls == 0) {
#pragma unroll
            for (int s = 1; s < QP; ++s)
                if (v[s] > best) { best = v[s]; lab = s; }            // strict: the lowest index wins a tie
        } else {
#pragma unroll 1
            for (int cl = 0; cl < d.ncls; ++cl) {
                float sum = 0.f;                                       // states in increasing index
#pragma unroll
                for (int s = 0; s < QP; ++s) sum = __builtin_fmaf(v[s], d.w[cl][s], sum);
                if (cl == 0 || sum > best) { best = sum; lab = cl; }
            }
        }
        const long long at = rowbase + tab[c] + row0 + r;
        __builtin_nontemporal_store((unsigned char)lab, d.label + at);
        if (d.conf) __builtin_nontemporal_store(best, d.conf + at);
    }
    __builtin_amdgcn_wave_barrier();
}

// ClassOut's flush: lane i takes row i % nrows of chain i / nrows as above and stores its ncls sums, ncls floats from
// 64-bit element offset (row index) * ncls.  The lanes of a store instruction write one float each, ncls floats
// apart; a row's line is completed by the same lane's next stores, so these are ordinary (cached) stores.
__device__ __forceinline__ void decode_rows(const OutStage &o, const ClassOut &d, long long rowbase, int lane, int row0,
                                            int nrows) {
    const float inv = 1.0f / (float)nrows;
    const int *tab = reinterpret_cast<const int *>(o.seg + 16 * OUT_STRIDE);
    __builtin_amdgcn_wave_barrier();
#pragma unroll 1                                                       // (one row's values in registers at a time)
    for (int pc = lane; pc < 16 * nrows; pc += 64) {
        const int c = (int)(((float)pc + 0.5f) * inv);                 // pc / nrows, exact for these ranges
        const int r = pc - c * nrows;
        if (r >= tab[16 + c] - row0) continue;                         // (a chain's ragged end; chains the wave does not own)
        const float *row = o.seg + c * OUT_STRIDE + r * o.q;
        float v[QP];
#pragma unroll
        for (int s = 0; s < QP; ++s) v[s] = s < o.q ? row[s] : 0.f;
        const long long at = (rowbase + tab[c] + row0 + r) * d.ncls;
#pragma unroll 1
        for (int cl = 0; cl < d.ncls; ++cl) {
            float sum = 0.f;                                           // states in increasing index
#pragma unroll
            for (int s = 0; s < QP; ++s) sum = __builtin_fmaf(v[s], d.w[cl][s], sum);
            if (d.prob) d.prob[at + cl] = sum;
            if (d.logp) d.logp[at + cl] = sum;
        }
    }
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ f4 log4(f4 v) {
    f4 r = {__logf(v.x), __logf(v.y), __logf(v.z), __logf(v.w)};
    return r;
}

// ---- coalesced emission loads.  In the tile layout the four lanes that hold one chain's row
// window (64 bytes) are 16 lanes apart, so a row load is 64 separate 16-byte L1 accesses
// (TCP_TOTAL_CACHE_ACCESSES: 501 M per k_forward launch against 111 M for the sparse reduce reading
// the same tensor).  Loader layout instead: lane -> (chain lane >> 2, piece lane & 3), adjacent
// lanes on adjacent 16-byte pieces, and the block is turned into the tile layout through
// wave-private LDS (one ds_write_b128 + one ds_read_b128 per row; chains IN_STRIDE floats apart
// puts both patterns on distinct banks).
#define IN_STRIDE (SUB * QP + 4)

__device__ __forceinline__ int loader_voff(const Tile &tl, int lane) {
    // byte offset of (chain lane >> 2, first row, piece lane & 3): lane c (g = 0) owns chain c's offset
    return __shfl(tl.voff, lane >> 2) + 16 * (lane & 3);
}
// rows[] (loader layout) -> e[] (tile layout: states 4g..4g+3 of chain n), through `seg`
template <int BS>
__device__ __forceinline__ void permute_rows(float *seg, int lane, int g, int n, const f4 (&rows)[BS], f4 (&e)[BS]) {
    constexpr int STRIDE = BS * QP + 4;
    float *wr = seg + (lane >> 2) * STRIDE + 4 * (lane & 3);
#pragma unroll
    for (int s = 0; s < BS; ++s) *reinterpret_cast<f4 *>(wr + s * QP) = rows[s];
    __builtin_amdgcn_wave_barrier();
    const float *rd = seg + n * STRIDE + 4 * g;
#pragma unroll
    for (int s = 0; s < BS; ++s) e[s] = *reinterpret_cast<const f4 *>(rd + s * QP);
    __builtin_amdgcn_wave_barrier();
}

// one exact forward cell step on the tile: X <- normalise(max(E,eps) * max(X A, eps))
__device__ __forceinline__ f4 fwd_step(const float (&af)[4], f4 X, f4 e, bool init, float eps, float *Sout) {
    f4 D = mfma4(af, X);
    f4 R = fmax4(sel4(init, X, D), eps);
    f4 sf = R * e;
    float S = col_sum(hsum(sf));
    float inv = __builtin_amdgcn_rcpf(S);
    *Sout = S;
    return sf * inv;
}

// ------------------------------------------------------------------ forward apply

// The apply kernels serve three plans.
//   KIND_SCAN   a wave owns 16 (sequence, chunk) pairs and starts from the chunk scan's prefix / suffix
//               vectors; models routed to the serial path (topo[m] == TOPO_EXACT) are skipped.
//   KIND_EXACT  (make_xplan) one chunk = the whole sequence, 16 sequences per wave, started from pi / ones
//               exactly as the cell's get_initial_state does (hmm_layer/MsaHmmCell.py:114-119) — the serial
//               recursion of the reference, step for step; only sequences whose verdict in `flags` is
//               ROUTE_WHOLE are computed and written.
//   KIND_WIN    a wave owns the windows (runs of chunks) of ONE flagged sequence, one window per tile
//               column: the same serial recursion over the window only, started from the exact vectors
//               the scan plan's kernels left at the window's two ends (see k_window_posterior).
//
// Which sequences leave the scan plan is decided on the device from psi, the posterior mass of
// clamp-born paths that the scan plan's backward kernel sums per chunk (backward_body); every serial
// kernel of a call reads the same verdict (k_exact_select): deterministic.
#define KIND_SCAN 0
#define KIND_EXACT 1
#define KIND_WIN 2
#define EXACT_DELTA 2e-6f       // a tenth of the posteriors' stated tolerance (2e-5)
#define ROUTE_NONE 0
#define ROUTE_WINDOWS 1
#define ROUTE_WHOLE 2
#define WIN_MAX 16                      // windows per sequence = tile columns (more: the whole sequence is redone)
#define WIN_STRIDE (2 * WIN_MAX + 2)    // ints per sequence in the window table: count, spare, (first chunk, chunks | lead << 24) pairs
#define WIN_LEAD (1 << 24)              // the window's forward pass starts one chunk early (at the flagged chunk itself)
#define WSH_STRIDE (WIN_MAX + WIN_MAX / 2)  // doubles per sequence in the shift table: WIN_MAX shifts, then WIN_MAX last chunks (ints)
static_assert(WSH_STRIDE == PLAN_WSH_STRIDE && WIN_STRIDE == PLAN_WIN_STRIDE, "plan strides");
static_assert(WIN_STRIDE == PLAN_WIN_STRIDE, "window table stride");
#define WIN_TOL 2e-6f                   // a window is accepted when its far-end vectors meet the scan plan's to this
#define WIN_MARGIN_STEPS 192            // how far past a flagged chunk a window reaches (rounded up to chunks)
struct Routing {
    const int *topo;
    int exact_mode;
    int *nexact;          // counter of routed sequences (kernels without a k_exact_select count themselves), or null
    const int *flags;     // per-sequence verdict (ROUTE_*) of k_exact_select, or null: per-model routing only
};
template <bool EXACT>
__device__ __forceinline__ bool route_tile(Tile &tl, int m, int g, const Routing &rt, float eps) {
    if (!EXACT) return rt.topo[m] != TOPO_EXACT;                     // wave-uniform: waves never straddle models
    bool need = tl.valid && rt.topo[m] == TOPO_EXACT;                // chain == sequence in the exact plan
    if (rt.flags) need = tl.valid && rt.flags[tl.chain] == ROUTE_WHOLE;
    tl.valid = need;
    tl.len = need ? tl.len : 0;
    if (rt.nexact && need && g == 0) atomicAdd(rt.nexact, 1);
    return __builtin_amdgcn_ballot_w64(need) != 0ull;
}

// checkpoint row of (this wave, block 0, chain n), states 4g..4g+3; block j is j * ckpt_block(p) floats on
__device__ __forceinline__ size_t ckpt_origin(const Tile &tl, const Plan &p, int g, int n) {
    return (((size_t)tl.wave * p.nsub) * p.cpw + n) * QP + 4 * g;
}
__device__ __forceinline__ size_t ckpt_block(const Plan &p) { return (size_t)p.cpw * QP; }

// a checkpoint row (read exactly once, by the wave that wrote it)
__device__ __forceinline__ f4 ld_ckpt(const float *ptr) {
#if HMM_CK_LD_NT
    return __builtin_nontemporal_load(reinterpret_cast<const f4 *>(ptr));
#else
    return *reinterpret_cast<const f4 *>(ptr);
#endif
}

// states 4g..4g+3 of a q-vector in the tile layout (0 beyond q)
__device__ __forceinline__ f4 ld_state4(const float *v, int q, int g) {
    f4 r;
    r.x = 4 * g + 0 < q ? v[4 * g + 0] : 0.f;
    r.y = 4 * g + 1 < q ? v[4 * g + 1] : 0.f;
    r.z = 4 * g + 2 < q ? v[4 * g + 2] : 0.f;
    r.w = 4 * g + 3 < q ? v[4 * g + 3] : 0.f;
    return r;
}
__device__ __forceinline__ f4 ones4(int q, int g) {
    f4 r = {4 * g + 0 < q ? 1.f : 0.f, 4 * g + 1 < q ? 1.f : 0.f, 4 * g + 2 < q ? 1.f : 0.f, 4 * g + 3 < q ? 1.f : 0.f};
    return r;
}
__device__ __forceinline__ f4 abs4(f4 v) {
    f4 r = {__builtin_fabsf(v.x), __builtin_fabsf(v.y), __builtin_fabsf(v.z), __builtin_fabsf(v.w)};
    return r;
}
// max(u, eps) with the sign bit set where the clamp was active (u <= eps): the flag costs one instruction more
// than the clamp itself
__device__ __forceinline__ f4 clamp_flag4(f4 u, float eps) {
    f4 r = {u.x > eps ? u.x : -eps, u.y > eps ? u.y : -eps, u.z > eps ? u.z : -eps, u.w > eps ? u.w : -eps};
    return r;
}
// component-wise with |.| as source modifiers (the packed multiply has none: written per component on purpose)
__device__ __forceinline__ f4 mul_abs4(f4 a, f4 b) {
    f4 r = {__builtin_fabsf(a.x) * b.x, __builtin_fabsf(a.y) * b.y, __builtin_fabsf(a.z) * b.z, __builtin_fabsf(a.w) * b.w};
    return r;
}
__device__ __forceinline__ float hsum_abs(f4 v) {
    return (__builtin_fabsf(v.x) + __builtin_fabsf(v.y)) + (__builtin_fabsf(v.z) + __builtin_fabsf(v.w));
}
// sum over the flagged (negative) components of a of |a| * w
__device__ __forceinline__ float flagged_dot(f4 a, f4 w) {
    float s = fmaxf(-a.x, 0.f) * w.x;
    s = fmaf(fmaxf(-a.y, 0.f), w.y, s);
    s = fmaf(fmaxf(-a.z, 0.f), w.z, s);
    return fmaf(fmaxf(-a.w, 0.f), w.w, s);
}
// sum of the negative components' magnitudes
__device__ __forceinline__ float hsum_neg(f4 v) {
    return (fmaxf(-v.x, 0.f) + fmaxf(-v.y, 0.f)) + (fmaxf(-v.z, 0.f) + fmaxf(-v.w, 0.f));
}

// WRITE_CKPT: alpha_hat entering every SUB-step block -> ck + j * ckb (posterior pipeline)
// WRITE_LOGA: log alpha -> out (forward_recursion)
// X: the vector entering the tile's first step (raw pi for a sequence's first chunk); ll0: the log-likelihood
//    up to there (log alpha output)
// KIND_EXACT / KIND_WIN also accumulate the log-likelihood of the steps walked, which is what the function returns
//    (every lane of a tile column holds it): the product of the normalisers c_t in fp64 with its exponent split off
//    once per block and ONE logarithm at the end — a window's value replaces the chunk scan's for its span, so it
//    has to be good to better than the clamp-born mass it accounts for (1e-6); per-step fp32 logarithms were not.
// Xend: alpha_hat after the tile's last step — after the last block (KIND_SCAN: meaningful for full chunks, the
//    only ones anybody reads), or captured at the block that ends the column's own window (KIND_WIN)
// CERT (scan plan of hmm_forward, which has no backward pass to sum psi in): the part of alpha_hat that descends
//    from the forward cell's clamps INSIDE this chunk is carried along as a second vector (Fv: the same step,
//    four more MFMAs) and weighed at the chunk's last position with the chunk scan's suffix vector there:
//    *cert = <Fv, suffix> / <alpha_hat, suffix> = the posterior mass of the paths born in this chunk — a path's
//    posterior mass is the same wherever it is measured, so the sum over a sequence's chunks is psi's forward half,
//    which is all that the log-likelihood and log alpha depend on.  WRITE_LOGA adds the clamp-born share of
//    alpha_hat itself at the chunk's end (log alpha is a statement about the filtered vector).
// BS: steps per block = checkpoint spacing (BS; the posterior's scan-plan pair may use 16)
template <bool WRITE_CKPT, bool WRITE_LOGA, int KIND, bool CERT = false, int BS = SUB>
__device__ __forceinline__ double forward_body(const float *__restrict__ A, const float *__restrict__ E, f4 X, double ll0,
                                             float *__restrict__ ck, size_t ckb, float *__restrict__ out,
                                             const Tile &tl, int m, float *seg, const Plan &p, float eps,
                                             f4 *Xend = nullptr, float *cert = nullptr, const float *sufv = nullptr) {
    const int lane = threadIdx.x & 63, g = lane >> 4, n = lane & 15;
    const int q = p.q;
    float af[4], ab[4];
    load_A(A + (size_t)m * q * q, q, g, n, af, ab);
    const Bounds bd = make_bounds(g, q, eps);
    const int rowb = q * (int)sizeof(float);
    constexpr bool ACC = WRITE_LOGA || KIND != KIND_SCAN;

    // `seg`: one LDS segment per wave: input permutation, and (log alpha) output staging — used in turn
    OutStage os;
    if (WRITE_LOGA)
        os = make_outstage(seg, reinterpret_cast<char *>(out + (tl.baseE - E)), q, lane, tl.voff - g * 16, tl.len);
    double llb = ll0;                                                 // log-likelihood up to the current block
    double dm = 1.0;                                                  // product of the normalisers, mantissa / exponent
    int de = 0;
    const f4 zero4c = {0.f, 0.f, 0.f, 0.f};
    f4 Fv = zero4c, Xc = X, Fc = zero4c;                              // CERT: clamp-born part of X; both at the chain's last step
    float shmax = 0.f;
    // the coalesced loader layout permutes through the LDS segment, which the log alpha variant
    // needs for its staged rows: that variant loads in the tile layout
    constexpr bool COAL = HMM_COALESCE_F && !WRITE_LOGA;
    int voff = COAL ? loader_voff(tl, lane) : tl.voff;
    f4 xe = X;

    // the next block's emission rows are in flight while the current block is computed
    // (the serial plans run one or two waves per SIMD with nothing else to hide a load behind: three blocks in flight)
    constexpr bool PF2 = HMM_FWD_PF2 || KIND != KIND_SCAN;
    f4 en[BS], en2[BS], en3[BS];
    ld_rows<BS>(tl.rsE, voff, rowb, en);
    if (PF2) {
        ld_rows<BS>(tl.rsE, voff + BS * rowb, rowb, en2);
        ld_rows<BS>(tl.rsE, voff + 2 * BS * rowb, rowb, en3);
    }
    for (int j = 0; j < p.nsub; ++j) {
#ifdef HMM_NT_CKPT
        if (WRITE_CKPT && tl.valid && j * BS < tl.len) __builtin_nontemporal_store(X, reinterpret_cast<f4 *>(ck + (size_t)j * ckb));
#else
        if (WRITE_CKPT && tl.valid && j * BS < tl.len) *reinterpret_cast<f4 *>(ck + (size_t)j * ckb) = X;
#endif
        f4 e[BS];
        if (COAL) {
            permute_rows<BS>(seg, lane, g, n, en, e);
        } else {
#pragma unroll
            for (int s = 0; s < BS; ++s) e[s] = en[s];
        }
        if (PF2) {
#pragma unroll
            for (int s = 0; s < BS; ++s) { en[s] = en2[s]; en2[s] = en3[s]; }
            if (j + 3 < p.nsub) ld_rows<BS>(tl.rsE, voff + 3 * BS * rowb, rowb, en3);
        } else {
            if (j + 1 < p.nsub) ld_rows<BS>(tl.rsE, voff + BS * rowb, rowb, en);
        }
        float lacc = 0.f;
#pragma unroll
        for (int s = 0; s < BS; ++s) {
            float S;
            if (CERT) {
                const bool init = tl.first && j == 0 && s == 0;
                const f4 ec = clampE(e[s], bd);
                const f4 D = mfma4(af, X), Df = mfma4(af, Fv);
                const f4 sf = fmax4(sel4(init, X, D), eps) * ec;
                f4 Rb = {D.x > eps ? Df.x : eps, D.y > eps ? Df.y : eps, D.z > eps ? Df.z : eps, D.w > eps ? Df.w : eps};
                Rb = sel4(init, Fv, Rb);                    // (the start distribution's own clamp: the scan has it)
                S = col_sum(hsum(sf));
                const float inv = __builtin_amdgcn_rcpf(S);
                X = sf * inv;
                Fv = Rb * ec * inv;
                const bool last = j * BS + s + 1 == tl.len;
                Xc = sel4(last, X, Xc);
                Fc = sel4(last, Fv, Fc);
            } else {
                X = fwd_step(af, X, clampE(e[s], bd), tl.first && j == 0 && s == 0, eps, &S);
            }
            if (WRITE_LOGA) {
                lacc += (j * BS + s < tl.len) ? __logf(S) : 0.f;
                float base = (float)(llb + (double)lacc);
                stage_row(os, n, g, (j % (HMM_OUT_ROWS / BS)) * BS + s, log4(X) + base);
            }
            if (KIND != KIND_SCAN) dm *= (j * BS + s < tl.len) ? (double)S : 1.0;
        }
        if (WRITE_LOGA) llb += (double)lacc;
        if (KIND != KIND_SCAN) { de += __builtin_amdgcn_frexp_exp(dm); dm = __builtin_amdgcn_frexp_mant(dm); }
        if (KIND == KIND_WIN) xe = sel4((j + 1) * BS == tl.len, X, xe);
        if (WRITE_LOGA && ((j + 1) % (HMM_OUT_ROWS / BS) == 0 || j + 1 == p.nsub))
            flush_rows(os, lane, (j / (HMM_OUT_ROWS / BS)) * HMM_OUT_ROWS, (j % (HMM_OUT_ROWS / BS) + 1) * BS);
        voff += BS * rowb;
    }
    if (Xend) *Xend = KIND == KIND_WIN ? xe : X;
    if (CERT) {
        const f4 sv = *reinterpret_cast<const f4 *>(sufv + 4 * g);
        const float num = col_sum(hsum(Fc * sv)), den = col_sum(hsum(Xc * sv));
        // log alpha: also the clamp-born share of alpha_hat itself where the chunk hands over to the next one (what
        // was born and forgotten inside the chunk the in-chunk steps have exactly; what is still there at the end is
        // missing from the next chunk's prefix)
        if (WRITE_LOGA) shmax = col_sum(hsum(Fc));
        // ... and what that share becomes one step on, under the NEXT observation (the first row of the chunk after,
        // whose kernel starts from the chunk scan's prefix vector: alpha_hat without its clamp-born part) — the mirror
        // image of backward_body's shnext
        float shnext = 0.f;
        if (WRITE_LOGA) {
            f4 en1 = {0.f, 0.f, 0.f, 0.f};
            const bool more = tl.valid && tl.chain % p.C != p.C - 1;             // (not the sequence's last chunk)
            if (more) {
                f4 r1[1];
                ld_rows<1>(tl.rsE, tl.voff + tl.len * rowb, rowb, r1);
                en1 = clampE(r1[0], bd);
            }
            const f4 Dx = fmax4(mfma4(af, Xc), eps), Df = mfma4(af, Fc);
            const float dn = col_sum(hsum(en1 * Dx));
            shnext = (more && dn > 0.f) ? col_sum(hsum(en1 * Df)) * __builtin_amdgcn_rcpf(dn) : 0.f;
        }
        *cert = fmaxf(fmaxf(num * __builtin_amdgcn_rcpf(den), shmax), shnext);
    }
    // the serial kernels of every entry point return the same value for the same sequence
    if (KIND != KIND_SCAN) return ll0 + log(dm) + (double)de * LN2;
    return llb;
}

// xend (scan plan, posterior pipeline): alpha_hat after every chain's last step, [chain][QP] — what a window of
// the serial recomputation starts from and is checked against
// CERT: psi[chain] = the chunk's clamp-born posterior mass (see forward_body), weighed with suffix[chain]
template <bool WRITE_CKPT, bool WRITE_LOGA, bool EXACT, bool CERT = false, int BS = SUB>
__global__ __launch_bounds__(256) void k_forward(const float *__restrict__ A, const float *__restrict__ pi,
                                                 const float *__restrict__ E,
                                                 const float *__restrict__ prefix, const double *__restrict__ llpre,
                                                 float *__restrict__ ckpt, float *__restrict__ out,
                                                 double *__restrict__ loglik, float *__restrict__ xend, Routing rt,
                                                 Plan p, float eps, long long nwaves, float *__restrict__ psi = nullptr,
                                                 const float *__restrict__ suffix = nullptr) {
    const long long wave = (long long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (wave >= nwaves) return;
    const int lane = threadIdx.x & 63, g = lane >> 4, n = lane & 15;
    int m; long long wc0;
    Tile tl = make_tile(E, p, wave, g, n, &m, &wc0);
    if (!route_tile<EXACT>(tl, m, g, rt, eps)) return;
    // LDS per wave: the staged log alpha rows, or only the input permutation's block
    constexpr int SEG = WRITE_LOGA ? OUT_SEG : 16 * (BS * QP + 4);
    __shared__ __attribute__((aligned(16))) float ostage[4 * SEG];
    float *seg = ostage + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) * SEG;
    const f4 X0 = EXACT ? ld_state4(pi + (size_t)m * p.q, p.q, g)
                        : *reinterpret_cast<const f4 *>(prefix + (size_t)tl.chain * QP + 4 * g);
    const double ll0 = (!EXACT && WRITE_LOGA) ? llpre[tl.chain] : 0.0;
    float *ck = ckpt + ckpt_origin(tl, p, g, n);
    f4 xe;
    float cert = 0.f;
    const double ll = forward_body<WRITE_CKPT, WRITE_LOGA, EXACT ? KIND_EXACT : KIND_SCAN, CERT, BS>(
        A, E, X0, ll0, ck, ckpt_block(p), out, tl, m, seg, p, eps, &xe, &cert,
        CERT ? suffix + (size_t)tl.chain * QP : nullptr);
    if (EXACT && tl.valid && g == 0) loglik[tl.chain] = ll;
    if (!EXACT && xend && tl.valid) *reinterpret_cast<f4 *>(xend + (size_t)tl.chain * QP + 4 * g) = xe;
    if (CERT && tl.valid && g == 0) psi[tl.chain] = cert;
}

// ------------------------------------------------------------------ backward apply

// MODE 0: gamma, 1: log gamma, 2: log gamma + loglik, 3: log beta (no forward part)
//
// psi (KIND_SCAN, MODE < 3): per chain, the posterior mass of CLAMP-BORN paths.  The chunk operators are the
// exactly linear products of A diag(E_t); the cell additionally lifts every component of the predicted state
// mixture to eps (hmm_layer/MsaHmmCell.py:87-88) in both directions.  The mass a clamp creates at (t, j) is
// part of alpha_hat_t[j] (forward cell) or of R_t[j] (reverse cell); paths through it carry the posterior weight
// gamma_t[j] at most, and that weight is the same at every position of the sequence (a path's posterior mass does
// not depend on where it is measured).  So psi = sum_t sum_{j: a prediction into (t, j) was clamped} gamma_t[j]
// bounds, for the WHOLE sequence, how far the serial recursion's posteriors and log-likelihood can be from the
// clamp-free scan's — and on the fp64 model the bound is attained (tools/experiments/cert_study.py: |d gamma| = psi
// to two digits).  The flags travel in the sign bits of the recomputed alpha_hat and of R, so the sign of their
// product marks a component that exactly one of the two clamps touched (one touched by both weighs eps^2 against
// sums of order eps at least: nothing), and psi's share of a step is the sum of the negative products: ~20 VALU
// per step in a kernel that waits for memory.
// Rend: R after the tile's first position has been walked = the vector leaving the chunk before.
// CERT3 (scan plan of hmm_backward, MODE 3: no forward part to take gamma from): the mirror image of forward_body's
// CERT — the part of R that descends from the reverse cell's clamps inside this chunk is carried along (Gv) and
// weighed at the chunk's FIRST position with alpha_hat there, one forward step from the chunk scan's prefix vector
// (prev): psi[chain] = <alpha_hat, Gv> / <alpha_hat, R> there, or the clamp-born share of the backward vector
// itself where the chunk hands over to the one before, if that is larger (log beta is a statement about that vector).
// DEC: the output policy (MODE 0): NoDecode stores the gamma rows, Decode their class labels, ClassOut their class sums
// (decode_rows); everything up to the staged rows is shared.
template <int MODE, int KIND, bool CERT3 = false, int BS = SUB, class DEC = NoDecode>
__device__ __forceinline__ void backward_body(const float *__restrict__ A, const float *__restrict__ E, f4 Rv, double lbb0,
                                              float llf, const float *__restrict__ ck, size_t ckb,
                                              float *__restrict__ out, float *__restrict__ psi, const Tile &tl, int m,
                                              float *seg, const Plan &p, float eps, f4 *Rend = nullptr,
                                              const float *prev = nullptr, double *lbb_end = nullptr,
                                              const DEC &dec = DEC()) {
    static_assert(!DEC::on || MODE == 0, "labels are decoded from the probability output");
    static_assert(HMM_OUT_ROWS % BS == 0, "a flush group holds whole blocks (HMM_OUT_ROWS / BS divides the block index)");
    const int lane = threadIdx.x & 63, g = lane >> 4, n = lane & 15;
    const int q = p.q;
    float af[4], ab[4];
    load_A(A + (size_t)m * q * q, q, g, n, af, ab);
    const Bounds bd = make_bounds(g, q, eps);
    const int rowb = q * (int)sizeof(float);
    // (Decode: the chain table in rows, not bytes, and the wave's first row in place of a base pointer)
    const OutStage os = DEC::on ? make_outstage(seg, nullptr, q, lane, (tl.voff - g * 16) / rowb, tl.len)
                                : make_outstage(seg, reinterpret_cast<char *>(out + (tl.baseE - E)), q, lane,
                                                tl.voff - g * 16, tl.len);
    const long long rowbase = DEC::on ? (long long)(tl.baseE - E) / q : 0;
    constexpr bool PSI = HMM_PSI && KIND == KIND_SCAN && MODE != 3;

    double lbb = lbb0;                                                // log scale of beta after the current block
    float ps = 0.f;
    if (MODE != 2) llf = 0.f;
    const f4 zero4g = {0.f, 0.f, 0.f, 0.f};
    f4 Gv = zero4g, Rc = Rv, Gc = zero4g, ec0 = zero4g;               // CERT3: clamp-born part of R; R, Gv, E at the first position
    float shmax = 0.f;

#if HMM_COALESCE_B
    const int lvoff = loader_voff(tl, lane);
#else
    const int lvoff = tl.voff;
#endif
    const f4 zero4 = {0.f, 0.f, 0.f, 0.f};
    f4 Xn = zero4;              // checkpoint of the block about to be processed, also prefetched
    if (MODE != 3 && tl.valid && (p.nsub - 1) * BS < tl.len)
        Xn = ld_ckpt(ck + (size_t)(p.nsub - 1) * ckb);

    // one BS-step block: recompute alpha_hat from the block's checkpoint, walk the backward steps,
    // stage the outputs; er = the block's raw emission rows
    // FULL: every chain of the wave owns all p.nsub * BS steps (all waves but those holding a sequence's last
    // chunk): no per-lane "is this step mine" selects
    auto block = [&](auto fullc, int j, const f4 *er) __attribute__((always_inline)) {
        constexpr bool FULL = decltype(fullc)::value;
        int srow = (j % (HMM_OUT_ROWS / BS)) * BS;                     // where this block's rows sit in the staged group
#if HMM_STAGE_BF
        // With BS == HMM_OUT_ROWS this is the constant 0 and the 4 * BS selected row addresses of stage_row are the
        // same in every block: hoisted out of the block loop they cost k_backward<0, ., ., 16> 50 registers and its
        // second wave per SIMD.  Opaque here, they are formed next to their writes.
        asm volatile("" : "+s"(srow));
#endif
        f4 e[BS];
#pragma unroll
        for (int s = 0; s < BS; ++s) e[s] = clampE(er[s], bd);
        const f4 Xc = Xn;
        if (j > 0 && MODE != 3 && tl.valid && (j - 1) * BS < tl.len)
            Xn = ld_ckpt(ck + (size_t)(j - 1) * ckb);
        f4 fa[BS];
        if (MODE != 3) {
            f4 X = Xc;
#pragma unroll
            for (int s = 0; s < BS; ++s) {
                const bool init = tl.first && j == 0 && s == 0;
                const f4 D = mfma4(af, X);
                if (PSI) {
                    // (the start distribution's own clamp is part of the scan's first vector: no flag)
                    const f4 Rf = sel4(init, fmax4(X, eps), clamp_flag4(D, eps));
                    const f4 sf = Rf * e[s];
                    fa[s] = sf * __builtin_amdgcn_rcpf(col_sum(hsum_abs(sf)));
                    X = abs4(fa[s]);
                } else {
                    const f4 sf = fmax4(sel4(init, X, D), eps) * e[s];
                    X = sf * __builtin_amdgcn_rcpf(col_sum(hsum(sf)));
                    fa[s] = X;
                }
            }
        }
        float lacc = 0.f;
#pragma unroll
        for (int s = BS - 1; s >= 0; --s) {
            const bool act = FULL || j * BS + s < tl.len;
            // gamma's normaliser Sg and the backward normaliser S both hang on Rv alone: summed as a pair
            constexpr bool PAIR = HMM_COLSUM2 && MODE != 3;
            const f4 sf = PSI ? mul_abs4(Rv, e[s]) : e[s] * Rv;
            float S;
            if (MODE == 3) {
                float base = (float)(lbb + (double)lacc);
                stage_row(os, n, g, srow + s, log4(Rv) + base);
            } else {
                f4 gm = fa[s] * Rv;                     // PSI: negative where exactly one of the two clamps was active
                float Sg;
                if (PAIR) col_sum2(PSI ? hsum_abs(gm) : hsum(gm), hsum(sf), Sg, S);
                else Sg = col_sum(PSI ? hsum_abs(gm) : hsum(gm));
                const float ig = __builtin_amdgcn_rcpf(Sg);
                if (PSI) ps = fmaf(hsum_neg(gm), act ? ig : 0.f, ps);
                if (MODE == 0) {
                    gm = PSI ? mul_abs4(gm, f4{ig, ig, ig, ig}) : gm * ig;
                } else {
                    gm = log4(PSI ? abs4(gm) : gm) - (__logf(Sg) - llf);
                }
                stage_row(os, n, g, srow + s, gm);
            }
            if (CERT3 && s == 0) { Rc = Rv; Gc = Gv; ec0 = e[0]; }   // (the last block executed is the chunk's first)
            if (!PAIR) S = col_sum(hsum(sf));
            const float iS = __builtin_amdgcn_rcpf(S);
            f4 bh = sf * iS;
            const f4 U = mfma4(ab, bh);
            const f4 Rn = PSI ? clamp_flag4(U, eps) : fmax4(U, eps);
            if (CERT3) {
                const f4 Ug = mfma4(ab, e[s] * Gv * iS);
                const f4 Gn = {U.x > eps ? Ug.x : eps, U.y > eps ? Ug.y : eps, U.z > eps ? Ug.z : eps, U.w > eps ? Ug.w : eps};
                Gv = sel4(act, Gn, Gv);
            }
            Rv = sel4(act, Rn, Rv);
            if (MODE == 3) lacc += act ? __logf(S) : 0.f;
        }
        if (MODE == 3) lbb += (double)lacc;
        if (j % (HMM_OUT_ROWS / BS) == 0) {                 // the group's earliest block is done: rows j*BS .. (top group: fewer)
            const int top = p.nsub - j;
            const int nrows = (top < (HMM_OUT_ROWS / BS) ? top : (HMM_OUT_ROWS / BS)) * BS;
            if constexpr (DEC::on) decode_rows(os, dec, rowbase, lane, j * BS, nrows);
            else flush_rows(os, lane, j * BS, nrows);
        }
    };

    const bool full = HMM_BWD_FULL && KIND == KIND_SCAN &&
                      __builtin_amdgcn_ballot_w64(tl.valid && tl.len != p.nsub * BS) == 0ull;
    // the previous (earlier-in-time) block's emission rows are in flight while this one is computed
    constexpr bool PF2 = KIND != KIND_SCAN;       // serial plans: two blocks in flight (see forward_body)
    f4 en[BS], en2[BS];
    ld_rows<BS>(tl.rsE, lvoff + (p.nsub - 1) * BS * rowb, rowb, en);
    if (PF2 && p.nsub > 1) ld_rows<BS>(tl.rsE, lvoff + (p.nsub - 2) * BS * rowb, rowb, en2);
    for (int j = p.nsub - 1; j >= 0; --j) {
        f4 e[BS];
#if HMM_COALESCE_B
        permute_rows<BS>(seg, lane, g, n, en, e);
#else
#pragma unroll
        for (int s = 0; s < BS; ++s) e[s] = en[s];
#endif
        if (PF2) {
#pragma unroll
            for (int s = 0; s < BS; ++s) en[s] = en2[s];
            if (j > 1) ld_rows<BS>(tl.rsE, lvoff + (j - 2) * BS * rowb, rowb, en2);
        } else if (j > 0) ld_rows<BS>(tl.rsE, lvoff + (j - 1) * BS * rowb, rowb, en);
        if (full) block(std::true_type(), j, e);
        else block(std::false_type(), j, e);
    }
    if (PSI) {
        ps = col_sum(ps);
        if (g == 0 && tl.valid) psi[tl.chain] = ps;
    } else if (KIND == KIND_SCAN && MODE != 3 && psi && g == 0 && tl.valid) {
        psi[tl.chain] = 0.f;
    }
    if (CERT3) {
        // alpha_hat at the chunk's first position, up to scale: one forward step from the vector entering the chunk
        const f4 P = *reinterpret_cast<const f4 *>(prev + 4 * g);
        const f4 a0 = fmax4(sel4(tl.first, P, mfma4(af, P)), eps) * ec0;
        const float num = col_sum(hsum(a0 * Gc)), den = col_sum(hsum(a0 * Rc));
        shmax = col_sum(hsum(Gv)) * __builtin_amdgcn_rcpf(col_sum(hsum(Rv)));      // what the chunk before does not get
        // ... and what that share becomes under the NEXT observation (the last row of the chunk before, whose kernel starts
        // from the chunk scan's suffix vector: the same direction without the floor).  A floor component that weighs 1e-16
        // here is all there is after a row that only its state can emit.
        float shnext = 0.f;
        {
            f4 ep = {0.f, 0.f, 0.f, 0.f};
            if (tl.valid && tl.chain % p.C != 0) {                  // (not the sequence's first chunk: the row exists)
                const char *pe = reinterpret_cast<const char *>(tl.baseE) + (tl.voff - rowb);
                const f4u raw = *reinterpret_cast<const f4u *>(pe);
                ep = clampE((f4){raw.x, raw.y, raw.z, raw.w}, bd);
            }
            const float dn = col_sum(hsum(ep * Rv));
            shnext = dn > 0.f ? col_sum(hsum(ep * Gv)) * __builtin_amdgcn_rcpf(dn) : 0.f;
        }
        const float c = fmaxf(fmaxf(num * __builtin_amdgcn_rcpf(den), shmax), shnext);
        if (g == 0 && tl.valid) psi[tl.chain] = c;
    }
    if (Rend) *Rend = PSI ? abs4(Rv) : Rv;
    if (MODE == 3 && lbb_end) *lbb_end = lbb;                 // log scale of beta after the tile's first position
}

// psi: [nchains]; rstart: R after every chain's first position, [chain][QP]
template <int MODE, bool EXACT, bool CERT3 = false, int BS = SUB>
__global__ __launch_bounds__(256) void k_backward(const float *__restrict__ A, const float *__restrict__ E,
                                                  const float *__restrict__ ckpt, const float *__restrict__ suffix,
                                                  const double *__restrict__ lsuf, const double *__restrict__ loglik,
                                                  float *__restrict__ out, float *__restrict__ psi,
                                                  float *__restrict__ rstart, Routing rt,
                                                  Plan p, float eps, long long nwaves,
                                                  const float *__restrict__ prefix = nullptr) {
    const long long wave = (long long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (wave >= nwaves) return;
    const int lane = threadIdx.x & 63, g = lane >> 4, n = lane & 15;
    int m; long long wc0;
    Tile tl = make_tile(E, p, wave, g, n, &m, &wc0);
    if (!route_tile<EXACT>(tl, m, g, rt, eps)) return;
    __shared__ __attribute__((aligned(16))) float ostage[4 * OUT_SEG];
    float *seg = ostage + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) * OUT_SEG;
    // the reverse cell's initial state: ones (hmm_layer/MsaHmmCell.py:115-116), or the chunk scan's suffix
    const f4 R0 = EXACT ? ones4(p.q, g) : *reinterpret_cast<const f4 *>(suffix + (size_t)tl.chain * QP + 4 * g);
    const double lbb0 = (MODE == 3 && !EXACT) ? lsuf[tl.chain] : 0.0;
    const float llf = MODE == 2 ? (float)loglik[tl.chain / p.C] : 0.f;
    const float *ck = ckpt + ckpt_origin(tl, p, g, n);
    f4 re;
    backward_body<MODE, EXACT ? KIND_EXACT : KIND_SCAN, CERT3, BS>(A, E, R0, lbb0, llf, ck, ckpt_block(p), out, psi, tl, m, seg,
                                                               p, eps, &re, CERT3 ? prefix + (size_t)tl.chain * QP : nullptr);
    if (!EXACT && rstart && tl.valid) *reinterpret_cast<f4 *>(rstart + (size_t)tl.chain * QP + 4 * g) = re;
}

// k_backward<0, false, false, BS> with the Decode output policy (hmm_posterior_decode) or ClassOut (hmm_class_posterior)
// (two blocks per compute unit, as k_backward<0> reaches on its own: at 16 steps per block the kernel sits at the edge
// of the 256 registers that allows, and the decode flush must not tip it over)
template <int BS, class DEC = Decode>
__global__ __launch_bounds__(256, 2) void k_backward_decode(const float *__restrict__ A, const float *__restrict__ E,
                                                         const float *__restrict__ ckpt, const float *__restrict__ suffix,
                                                         float *__restrict__ psi, float *__restrict__ rstart, Routing rt,
                                                         Plan p, float eps, long long nwaves, const DEC dec) {
    const long long wave = (long long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (wave >= nwaves) return;
    const int lane = threadIdx.x & 63, g = lane >> 4, n = lane & 15;
    int m; long long wc0;
    Tile tl = make_tile(E, p, wave, g, n, &m, &wc0);
    if (!route_tile<false>(tl, m, g, rt, eps)) return;
    __shared__ __attribute__((aligned(16))) float ostage[4 * OUT_SEG];
    float *seg = ostage + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) * OUT_SEG;
    const f4 R0 = *reinterpret_cast<const f4 *>(suffix + (size_t)tl.chain * QP + 4 * g);
    const float *ck = ckpt + ckpt_origin(tl, p, g, n);
    f4 re;
    backward_body<0, KIND_SCAN, false, BS, DEC>(A, E, R0, 0.0, 0.f, ck, ckpt_block(p), nullptr, psi, tl, m, seg, p, eps,
                                                &re, nullptr, nullptr, dec);
    if (rstart && tl.valid) *reinterpret_cast<f4 *>(rstart + (size_t)tl.chain * QP + 4 * g) = re;
}

// ---- the per-sequence verdict, one wave per sequence.
//   ROUTE_WHOLE    model routed by k_topo_check; or too much of the sequence is flagged
//   ROUTE_WINDOWS  psi (summed over the sequence's chunks) above EXACT_DELTA: the chunks that carry the
//                  clamp-born mass are found, each is widened by `margin` chunks on either side (forward-born mass
//                  changes alpha_hat downstream, backward-born mass R upstream), overlapping runs are merged -> the
//                  window table; the rest of the sequence keeps the scan's values
//   ROUTE_NONE     everything else
// wcnt: [0] sequences with windows (= entries of wlist), [1] sequences redone whole because of their psi or of
// windows that ran into each other, [2] windows, [3] chunks the windows walked; zeroed by k_topo_check.
// exps (or null): the chunk operators' exponent rows; the sparse reduce marks chains whose columns went through the
// denormal range there (reduce_sparse_wave's `risk`) — such a chunk counts as flagged whatever its psi
__global__ __launch_bounds__(64) void k_exact_select(const int *__restrict__ topo, float *__restrict__ psi, Plan p,
                                                     int exact_mode, int margin, int *__restrict__ flags,
                                                     int *__restrict__ nexact, int *__restrict__ wtab,
                                                     int *__restrict__ wlist, int *__restrict__ wcnt,
                                                     const int *__restrict__ exps = nullptr,
                                                     const float *__restrict__ prefix = nullptr,
                                                     const float *__restrict__ rstart = nullptr, float eps = 0.f) {
    const int seq = blockIdx.x, lane = threadIdx.x;
    const int C = p.C;
    const int tpv = topo[seq / p.b];
    if (tpv == TOPO_EXACT) {
        if (lane == 0) { flags[seq] = ROUTE_WHOLE; atomicAdd(nexact, 1); }
        return;
    }
    float *pc = psi + (size_t)seq * C;
    // prefix, rstart (the posterior's scan plan): the reverse cell's clamp where chunk c hands over to chunk c - 1.
    // backward_body clamps and flags the vector that leaves chunk c (rstart[c], R at the last position of chunk c - 1),
    // but the gamma that weighs those flags belongs to chunk c - 1, whose kernel starts from the chunk scan's suffix
    // vector: the same direction without the clamp.  Neither kernel sums that term; it is summed here, with alpha_hat
    // at that position (the chunk scan's prefix of chunk c), and charged to chunk c: chunk c itself is right, what
    // the birth changes is R before it, which is what a window before a flagged chunk recomputes from rstart[c].
    if (prefix && exact_mode == HMM_EXACT_AUTO)
        for (int c = lane; c < C; c += 64) {
            if (c == 0) continue;
            const float *a = prefix + ((size_t)seq * C + c) * QP, *r = rstart + ((size_t)seq * C + c) * QP;
            float born = 0.f, all = 0.f;
            for (int j = 0; j < p.q; ++j) {
                const float w = fabsf(a[j]) * r[j];
                all += w;
                born += r[j] <= eps ? w : 0.f;
            }
            if (born > 0.f) pc[c] += born / all;
        }
    if (exps && tpv != 0 && exact_mode == HMM_EXACT_AUTO)          // (every later loop visits chunk c from the same lane)
        for (int c = lane; c < C; c += 64)
            if (exps[((size_t)seq * C + c) * QP + QP - 1] != 0) pc[c] = 1.f;
    float s = 0.f;
    if (exact_mode == HMM_EXACT_AUTO) {
        for (int c = lane; c < C; c += 64) s += pc[c];
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    }
    if (s <= EXACT_DELTA) {                                           // (NaN / inf fall through)
        if (lane == 0) flags[seq] = ROUTE_NONE;
        return;
    }
    if (margin < 0) {                                                 // this entry point has no windows
        if (lane == 0) { flags[seq] = ROUTE_WHOLE; atomicAdd(nexact, 1); atomicAdd(wcnt + 1, 1); }
        return;
    }
    // the largest per-chunk threshold that leaves at most EXACT_DELTA / 2 outside the flagged chunks
    float thr = EXACT_DELTA * 0.125f;
    for (int it = 0; it < 8; ++it) {
        float rem = 0.f;
        for (int c = lane; c < C; c += 64) { const float v = pc[c]; rem += v <= thr ? v : 0.f; }
        for (int o = 32; o > 0; o >>= 1) rem += __shfl_xor(rem, o);
        if (rem <= 0.5f * EXACT_DELTA) break;
        thr *= 0.125f;
    }
    // Windows.  A flagged chunk c standing alone is itself right as the scan plan computed it — its in-chunk steps
    // apply the clamps, from vectors that are right when nothing flagged precedes / follows within reach; what its
    // births change is alpha_hat AFTER it and R BEFORE it.  It therefore gets two windows, [c - margin, c - 1] and
    // [c + 1, c + margin] (two tile columns of the window kernel: they run side by side); the second one's forward
    // pass starts at c itself (WIN_LEAD) so that the window's log-likelihood covers the births inside c.  A run of
    // adjacent flagged chunks becomes one window with the margin on either side.  Windows that touch are merged.
    __shared__ int wlo[WIN_MAX], whi[WIN_MAX], wld[WIN_MAX];
    int nw = 0;
    bool over = false;
    auto push = [&](int lo, int hi, int lead) {                       // lane 0 only
        while (nw > 0 && lo <= whi[nw - 1] + 1) {
            const int fstart = min(lo - lead, wlo[nw - 1] - wld[nw - 1]);     // where the merged forward pass starts
            lo = min(lo, wlo[nw - 1]); hi = max(hi, whi[nw - 1]); --nw;
            lead = lo - fstart;
        }
        if (nw == WIN_MAX) { over = true; lo = min(lo, wlo[nw - 1]); hi = max(hi, whi[nw - 1]); lead = wld[nw - 1]; --nw; }
        wlo[nw] = lo; whi[nw] = hi; wld[nw] = lead; ++nw;
    };
    auto flush_run = [&](int c, int d) {
        if (c < 0) return;
        if (d > c) { push(max(0, c - margin), min(C - 1, d + margin), 0); return; }
        if (c > 0) push(max(0, c - margin), c - 1, 0);
        push(c + 1, min(C - 1, c + margin), 1);                       // (c == C - 1: no chunks, the forward pass over c alone)
    };
    int run_lo = -1, run_hi = -2;
    for (int base = 0; base < C; base += 64) {
        const int c = base + lane;
        const bool hot = c < C && !(pc[c] <= thr);
        const unsigned long long hmask = __builtin_amdgcn_ballot_w64(hot);
        if (lane == 0) {
            unsigned long long any = hmask;
            while (any) {
                const int bit = __builtin_ctzll(any);
                any &= any - 1;
                const int cc = base + bit;
                if (cc == run_hi + 1) { run_hi = cc; }
                else { flush_run(run_lo, run_hi); run_lo = run_hi = cc; }
            }
        }
    }
    if (lane == 0) {
        flush_run(run_lo, run_hi);
        int tot = 0;
        for (int i = 0; i < nw; ++i) tot += whi[i] - wlo[i] + 1 + wld[i];
        const bool whole = over || 4ll * tot >= 3ll * C;
        flags[seq] = whole ? ROUTE_WHOLE : ROUTE_WINDOWS;
        atomicAdd(nexact, 1);
        if (whole) {
            atomicAdd(wcnt + 1, 1);
        } else {
            int *wt = wtab + (size_t)seq * WIN_STRIDE;
            wt[0] = nw;
            for (int i = 0; i < nw; ++i) { wt[2 + 2 * i] = wlo[i]; wt[3 + 2 * i] = (whi[i] - wlo[i] + 1) | (wld[i] ? WIN_LEAD : 0); }
            wlist[atomicAdd(wcnt, 1)] = seq;
            atomicAdd(wcnt + 2, nw);
        }
    }
}

// ---- windows: the serial recursion over the flagged runs of chunks only.  One wave per sequence with windows
// (grid stride over wlist), window i in tile column i.  A window [lo, hi] walks the cell's exact steps
//   forward   from alpha_hat at the end of chunk lo - 1 (xend: what the scan plan's forward kernel stepped to from a
//             prefix that no flagged chunk precedes within reach), and on PAST hi, a growing number of chunks at a
//             time, until the posterior it arrives with at a chunk's last position (its alpha_hat times the scan
//             plan's R there) equals the scan plan's to WIN_TOL — the births inside the window have then been
//             forgotten by the recursion, as far as the future can tell — or the sequence ends;
//   backward  from R at the start of chunk hi + 1 (rstart) over everything the forward pass walked, and on BELOW lo
//             (recomputing the scan's forward vectors there for the checkpoints) until the posterior before the
//             window (the scan plan's alpha_hat times its R) meets the scan plan's;
// and writes the outputs of every position it walked.  Everything outside stands as the scan computed it; the
// window's own log-likelihood takes the place of the chunk scan's for its forward span.  A window may grow up to
// its neighbours; one that has not met the scan's vectors by then (the windows would have to be merged) sends its
// sequence to the whole-sequence kernel that follows.  The cost of a flagged sequence is therefore the flagged
// chunks plus the model's forgetting time, not its length.  Checkpoints: rows [seq][chunk][block] of the checkpoint
// region (the scan plan's checkpoints have been consumed by k_backward).
// What a window does on its way back is the caller's (Pol): the posterior kernels' backward body, the gradient's
// (hmm_grad.inc), or nothing at all (log-likelihood only: MODE 4, the forward half alone — the windows' log-likelihood
// in place of the chunk scan's; the future's weights in the far-end check are then the chunk scan's suffix vectors).
//   Pol::BACKWARD, Pol::CKPT                       compile-time: is there a backward half, are checkpoints written
//   pol.backward(tl, m, R, ck, pw, &re)            walk tile tl backward from R (checkpoint rows ck + j * QP)
//   pol.finish(seq, good)                          after the sequence's windows (good: none ran into a neighbour)
// The final extents of the windows are written back to the table (the gradient's second scan-plan launch leaves
// exactly these chains out).
template <class Pol>
__device__ __forceinline__ void window_walk(Pol &pol, const float *__restrict__ A, const float *__restrict__ E,
                                            const float *__restrict__ prefix, const double *__restrict__ llpre,
                                            const float *__restrict__ suffix, const float *__restrict__ xend,
                                            const float *__restrict__ rstart, float *__restrict__ ckpt,
                                            double *__restrict__ loglik, int *__restrict__ wtab,
                                            const int *__restrict__ wlist, int *__restrict__ wcnt, int *__restrict__ flags,
                                            double *__restrict__ dfix, const Plan &p, float eps, int ext0, float *seg,
                                            double *__restrict__ wshift = nullptr) {
    constexpr bool LLONLY = !Pol::BACKWARD;
    constexpr bool LOGA = Pol::LOGA;       // the forward half also writes log alpha of what it walks (pol.loga)
    const int lane = threadIdx.x & 63, g = lane >> 4, n = lane & 15;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nlist = wcnt[0];
    const int C = p.C;
    const unsigned long long total = (unsigned long long)p.NB * p.L * p.q * sizeof(float);
    const f4 zero4 = {0.f, 0.f, 0.f, 0.f};
    auto wave_max = [](int v) {
        for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
        return __builtin_amdgcn_readfirstlane(v);
    };
    for (int it = blockIdx.x * 4 + w; it < nlist; it += gridDim.x * 4) {
        const int seq = wlist[it];
        const int m = seq / p.b;
        int *wt = wtab + (size_t)seq * WIN_STRIDE;
        const int nwin = wt[0];
        const bool valid = n < nwin;
        int lo = valid ? wt[2 + 2 * n] : 0;
        const int lead = valid && (wt[3 + 2 * n] & WIN_LEAD) ? 1 : 0;                 // the forward pass starts at lo - lead
        int hi = valid ? lo + (wt[3 + 2 * n] & (WIN_LEAD - 1)) - 1 : -1;
        const int lo_first = lo - lead;
        // where the next window's forward pass starts: this one's has to have met the scan's vectors by then
        const int lo_next = (valid && n + 1 < nwin) ? wt[2 + 2 * (n + 1)] - ((wt[3 + 2 * (n + 1)] & WIN_LEAD) ? 1 : 0) : C;
        const float *baseE = E + (size_t)seq * p.L * p.q;
        const __amdgpu_buffer_rsrc_t rs = make_rsrc(baseE, total - (unsigned long long)seq * p.L * p.q * sizeof(float));
        const size_t chs = (size_t)seq * C;                                          // chain of the sequence's chunk 0
        float *ckq = ckpt + chs * p.nsub * QP + 4 * g;
        const double ll_scan = loglik[seq];
        pol.begin(seq, m, (float)ll_scan);
        // what a column walks in one call: chunks [a, a + nch) (nothing when !on)
        auto seg_tile = [&](bool on, int a, int nch) {
            Tile tl;
            tl.wave = 0;
            tl.chain = (long long)(chs + (on ? a : 0));
            tl.valid = on;
            tl.first = on && a == 0 && p.seq_start;
            tl.len = on ? min(nch * p.T, p.L - a * p.T) : 0;
            tl.voff = (on ? a : 0) * p.T * p.q * (int)sizeof(float) + g * 16;
            tl.baseE = baseE;
            tl.rsE = rs;
            return tl;
        };
        auto ld4 = [&](bool on, const float *ptr) { return on ? *reinterpret_cast<const f4 *>(ptr + 4 * g) : zero4; };
        auto start_vec = [&](bool on, int a) {        // alpha_hat entering chunk a, as the scan plan has it
            return ld4(on, a == 0 ? prefix + chs * QP : xend + (chs + (on ? a : 1) - 1) * QP);
        };
        bool conflict = false;
        // ---- forward: the window, then on until the scan's vector is met
        f4 X = start_vec(valid, lo_first);
        double llw = 0.0;
        // log alpha_t = log alpha_hat_t + the log-likelihood up to t: the window's rows carry the chunk scan's value at
        // the window's start plus the window's own steps; what earlier windows of the sequence changed is added to
        // every later row afterwards (k_window_shift_loga)
        double llrun = (LOGA && valid) ? llpre[chs + lo_first] : 0.0;
        {
            bool on = valid, merged = !valid;
            int a = lo_first, nch = hi - lo_first + 1, ext = ext0;
            while (__builtin_amdgcn_ballot_w64(on) != 0ull) {
                const Tile tl = seg_tile(on, a, nch);
                Plan pw = p;
                pw.nsub = (wave_max(tl.len) + SUB - 1) / SUB;
                f4 xe;
                const double l = forward_body<Pol::CKPT, LOGA, KIND_WIN>(A, E, X, llrun, ckq + (size_t)(on ? a : 0) * p.nsub * QP,
                                                                        (size_t)QP, pol.loga(), tl, m, seg, pw, eps, &xe) - llrun;
                if (on) { X = xe; llw += l; llrun += l; hi = a + nch - 1; }
                const bool tail = hi + 1 >= C;
                // met = the POSTERIORS at the chunk's last position agree (the scan plan's R there weighs the
                // difference: a component that is tiny in alpha_hat may be all the future cares about — comparing
                // the filtered vectors alone accepted windows that were off by 6e-2 downstream)
                const bool chk = on && !tail;
                const f4 xs = ld4(chk, xend + (chs + (on ? hi : 0)) * QP);
                const f4 rw = ld4(chk, LLONLY ? suffix + (chs + (on ? hi : 0)) * QP : rstart + (chs + (on ? hi : 0) + 1) * QP);
                const f4 ge = X * rw, gs = xs * rw;
                const float ie = __builtin_amdgcn_rcpf(col_sum(hsum(ge))), is = __builtin_amdgcn_rcpf(col_sum(hsum(gs)));
                float d = col_max(hmax(abs4(ge * ie - gs * is)));
                if (LOGA) d = fmaxf(d, col_max(hmax(abs4(X - xs))));    // log alpha is a statement about alpha_hat itself
                if (on) merged = tail || d <= WIN_TOL;
                on = valid && !merged;
                if (on) {
                    a = hi + 1;
                    const int bnd = min(min(C - 1, lo_next - 1), a + ext - 1);
                    if (bnd < a) { conflict = true; on = false; }
                    nch = bnd - a + 1;
                }
                ext *= 2;
            }
        }
        double dll = 0.0;
        if (valid) dll = llw - ((hi + 1 >= C ? ll_scan : llpre[chs + hi + 1]) - llpre[chs + lo_first]);
        __threadfence();
        // ---- backward: everything the forward pass walked, then on below the window until the scan's R is met
        if (Pol::BACKWARD) {
            f4 R = ld4(valid, hi + 1 >= C ? suffix + (chs + max(hi, 0)) * QP : rstart + (chs + hi + 1) * QP);
            const bool nonempty = valid && hi >= lo;             // (a lead-only window at the sequence's end has no chunks)
            {
                const Tile tl = seg_tile(nonempty, lo, hi - lo + 1);
                Plan pw = p;
                pw.nsub = (wave_max(tl.len) + SUB - 1) / SUB;
                f4 re;
                pol.backward(A, E, tl, m, R, ckq + (size_t)(nonempty ? lo : 0) * p.nsub * QP, pw, eps, seg, &re);
                if (nonempty) R = re;
            }
            const int hi_prev = __shfl(hi, (lane + 63) & 63);        // the previous window's last chunk after its forward pass
            const int lob = (valid && n > 0) ? hi_prev + 1 : 0;
            bool merged = !nonempty;
            int ext = ext0;
            while (true) {
                // met = the posteriors at the last position BEFORE the window agree (weighed by the scan plan's
                // alpha_hat there)
                const bool chk = nonempty && lo > 0;
                const f4 rsv = ld4(chk, rstart + (chs + lo) * QP);
                const f4 aw = ld4(chk, xend + (chs + max(lo, 1) - 1) * QP);
                const f4 ge = aw * R, gs = aw * rsv;
                const float i1 = __builtin_amdgcn_rcpf(col_sum(hsum(ge))), i2 = __builtin_amdgcn_rcpf(col_sum(hsum(gs)));
                const float d = col_max(hmax(abs4(ge * i1 - gs * i2)));
                if (nonempty && !merged) merged = lo == 0 || d <= WIN_TOL;
                bool on = nonempty && !merged && !conflict;
                int a = 0, nch = 0;
                if (on) {
                    a = max(lob, lo - ext);
                    if (a > lo - 1) { conflict = true; on = false; }
                    nch = lo - a;
                }
                if (__builtin_amdgcn_ballot_w64(on) == 0ull) break;
                const Tile tl = seg_tile(on, a, nch);
                Plan pw = p;
                pw.nsub = (wave_max(tl.len) + SUB - 1) / SUB;
                float *ck = ckq + (size_t)(on ? a : 0) * p.nsub * QP;
                forward_body<true, false, KIND_WIN>(A, E, start_vec(on, a), 0.0, ck, (size_t)QP, nullptr, tl, m, seg, pw, eps);
                __threadfence();
                f4 re;
                pol.backward(A, E, tl, m, R, ck, pw, eps, seg, &re);
                if (on) { R = re; lo = a; }
                ext *= 2;
            }
        }
        const bool good = __builtin_amdgcn_ballot_w64(valid && conflict) == 0ull;
        // the sequence's log-likelihood: the windows' own sums in place of the chunk scan's, in window order
        double dsum = 0.0;
        int walked = 0;
        for (int i = 0; i < nwin; ++i) {
            const long long bits = __builtin_bit_cast(long long, dll);
            const int lo32 = __builtin_amdgcn_readlane((int)bits, i), hi32 = __builtin_amdgcn_readlane((int)(bits >> 32), i);
            dsum += __builtin_bit_cast(double, ((long long)hi32 << 32) | (unsigned int)lo32);
            walked += __builtin_amdgcn_readlane(hi - lo + 1, i);
        }
        if (valid && g == 0) { wt[2 + 2 * n] = lo; wt[3 + 2 * n] = hi - lo + 1; }     // the final extents (outputs written)
        if (wshift && valid && g == 0) {
            double *ws_ = wshift + (size_t)seq * WSH_STRIDE;
            ws_[n] = dll;
            reinterpret_cast<int *>(ws_ + WIN_MAX)[n] = hi;
        }
        // (a chunk scan that broke down altogether — a non-finite log-likelihood — cannot be repaired by differences)
        const bool fine = good && __builtin_isfinite(ll_scan + dsum);
        if (lane == 0) {
            atomicAdd(wcnt + 3, walked);
            if (fine) {
                loglik[seq] = ll_scan + dsum;
                dfix[seq] = dsum;
            } else {
                flags[seq] = ROUTE_WHOLE;
                atomicAdd(wcnt + 1, 1);
            }
        }
        pol.finish(seq, m, fine);
    }
}

// MODE 0..2: the posterior's output modes; MODE 4: the log-likelihood alone (hmm_forward without log alpha)
// MODE 5: log alpha (hmm_forward): forward half only, writing log alpha of every position walked
template <int MODE, class DEC = NoDecode>
struct PostWindows {
    static constexpr bool BACKWARD = MODE < 4, CKPT = MODE < 4, LOGA = MODE == 5;
    float *out;
    float llf;
    const DEC *dec = nullptr;   // Decode: the kernel's own argument (the weights stay in the argument segment)
    __device__ __forceinline__ float *loga() const { return LOGA ? out : nullptr; }
    __device__ __forceinline__ void begin(int, int, float ll_scan) { llf = ll_scan; }
    __device__ __forceinline__ void backward(const float *A, const float *E, const Tile &tl, int m, f4 R, const float *ck,
                                             const Plan &pw, float eps, float *seg, f4 *re) {
        if constexpr (DEC::on)
            backward_body<0, KIND_WIN, false, SUB, DEC>(A, E, R, 0.0, llf, ck, (size_t)QP, out, nullptr, tl, m, seg, pw, eps,
                                                        re, nullptr, nullptr, *dec);
        else
            backward_body<MODE >= 4 ? 0 : MODE, KIND_WIN>(A, E, R, 0.0, llf, ck, (size_t)QP, out, nullptr, tl, m, seg, pw, eps, re);
    }
    __device__ __forceinline__ void finish(int, int, bool) {}
};

template <int MODE>
__global__ __launch_bounds__(256) void k_window_posterior(const float *__restrict__ A, const float *__restrict__ E,
                                                          const float *__restrict__ prefix, const double *__restrict__ llpre,
                                                          const float *__restrict__ suffix, const float *__restrict__ xend,
                                                          const float *__restrict__ rstart, float *__restrict__ ckpt,
                                                          double *__restrict__ loglik, float *__restrict__ out,
                                                          int *__restrict__ wtab, const int *__restrict__ wlist,
                                                          int *__restrict__ wcnt, int *__restrict__ flags,
                                                          double *__restrict__ dfix, Plan p, float eps, int ext0,
                                                          double *__restrict__ wshift = nullptr) {
    constexpr int SEG = MODE == 4 ? 16 * IN_STRIDE : OUT_SEG;
    __shared__ __attribute__((aligned(16))) float ostage[4 * SEG];
    float *seg = ostage + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) * SEG;
    PostWindows<MODE> pol;
    pol.out = out;
    window_walk(pol, A, E, prefix, llpre, suffix, xend, rstart, ckpt, loglik, wtab, wlist, wcnt, flags, dfix, p, eps, ext0, seg,
                wshift);
}

// k_window_posterior<0> with the Decode output policy (hmm_posterior_decode) or ClassOut (hmm_class_posterior)
template <class DEC = Decode>
__global__ __launch_bounds__(256) void k_window_decode(const float *__restrict__ A, const float *__restrict__ E,
                                                       const float *__restrict__ prefix, const double *__restrict__ llpre,
                                                       const float *__restrict__ suffix, const float *__restrict__ xend,
                                                       const float *__restrict__ rstart, float *__restrict__ ckpt,
                                                       double *__restrict__ loglik, int *__restrict__ wtab,
                                                       const int *__restrict__ wlist, int *__restrict__ wcnt,
                                                       int *__restrict__ flags, double *__restrict__ dfix, Plan p, float eps,
                                                       int ext0, const DEC dec) {
    __shared__ __attribute__((aligned(16))) float ostage[4 * OUT_SEG];
    float *seg = ostage + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) * OUT_SEG;
    PostWindows<0, DEC> pol;
    pol.out = nullptr;
    pol.dec = &dec;
    window_walk(pol, A, E, prefix, llpre, suffix, xend, rstart, ckpt, loglik, wtab, wlist, wcnt, flags, dfix, p, eps, ext0, seg,
                nullptr);
}

// log beta (hmm_backward) of the sequences k_exact_select gave windows: the backward half alone.  What is born in a
// flagged chunk changes R BEFORE it; every window of the table is walked backward from the scan plan's
// R at its upper end (rstart) with the chunk scan's log scale there, writing log beta, and on below the
// window until the vector it arrives with equals the scan plan's — weighed with alpha_hat there as the chunk scan has
// it (hmm_backward's uniform start), and unweighed, log beta being a statement about the vector itself.  The rows
// BELOW a window then move with its log scale (k_window_shift_logb).  Windows that run into their neighbours send
// the sequence to the whole-sequence kernel.
__global__ __launch_bounds__(256) void k_window_logbeta(const float *__restrict__ A, const float *__restrict__ E,
                                                        const float *__restrict__ prefix, const float *__restrict__ suffix,
                                                        const double *__restrict__ lsuf, const float *__restrict__ rstart,
                                                        float *__restrict__ out, int *__restrict__ wtab,
                                                        const int *__restrict__ wlist, int *__restrict__ wcnt,
                                                        int *__restrict__ flags, double *__restrict__ wshift, Plan p,
                                                        float eps, int ext0) {
    __shared__ __attribute__((aligned(16))) float ostage[4 * OUT_SEG];
    float *seg = ostage + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) * OUT_SEG;
    const int lane = threadIdx.x & 63, g = lane >> 4, n = lane & 15;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nlist = wcnt[0];
    const int C = p.C;
    const unsigned long long total = (unsigned long long)p.NB * p.L * p.q * sizeof(float);
    const f4 zero4 = {0.f, 0.f, 0.f, 0.f};
    auto wave_max = [](int v) {
        for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
        return __builtin_amdgcn_readfirstlane(v);
    };
    for (int it = blockIdx.x * 4 + w; it < nlist; it += gridDim.x * 4) {
        const int seq = wlist[it];
        const int m = seq / p.b;
        int *wt = wtab + (size_t)seq * WIN_STRIDE;
        const int nwin = wt[0];
        const bool valid = n < nwin;
        int lo = valid ? wt[2 + 2 * n] : 0;
        const int hi_tab = valid ? lo + (wt[3 + 2 * n] & (WIN_LEAD - 1)) - 1 : -1;
        // (every window is walked: one that only follows a flagged chunk meets the scan's R at once, but merged windows
        // carry the lead mark of their first part)
        const bool act = valid && hi_tab >= lo;
        // the pass starts one chunk ABOVE the window: a flagged chunk standing alone sits there (its own rows are
        // right as the scan computed them, but the log scale it hands down has to be the in-chunk one; the mirror
        // image of WIN_LEAD) — any other chunk is simply walked again with the same result
        const int hi = act ? min(hi_tab + 1, C - 1) : hi_tab;
        const float *baseE = E + (size_t)seq * p.L * p.q;
        const __amdgpu_buffer_rsrc_t rs = make_rsrc(baseE, total - (unsigned long long)seq * p.L * p.q * sizeof(float));
        const size_t chs = (size_t)seq * C;
        auto seg_tile = [&](bool on, int a, int nch) {
            Tile tl;
            tl.wave = 0;
            tl.chain = (long long)(chs + (on ? a : 0));
            tl.valid = on;
            tl.first = on && a == 0 && p.seq_start;
            tl.len = on ? min(nch * p.T, p.L - a * p.T) : 0;
            tl.voff = (on ? a : 0) * p.T * p.q * (int)sizeof(float) + g * 16;
            tl.baseE = baseE;
            tl.rsE = rs;
            return tl;
        };
        auto ld4 = [&](bool on, const float *ptr) { return on ? *reinterpret_cast<const f4 *>(ptr + 4 * g) : zero4; };
        // the window itself, from R at the last position of chunk hi as the chunk above left it (rstart: the in-chunk
        // steps' normalisation, every component lifted to eps as the cell does — the chunk scan's suffix vector is the
        // same direction WITHOUT the floor, which is all that is left of some states inside a stretch); its log scale
        // is the suffix vector's, moved by the ratio of the two vectors' sums.  The sequence's last chunk starts from
        // the suffix vector itself (ones).
        const bool top = hi + 1 >= C;
        const f4 sv0 = ld4(act, suffix + (chs + max(hi, 0)) * QP);
        f4 R = top ? sv0 : ld4(act, rstart + (chs + hi + 1) * QP);
        double lbrun = 0.0;
        {
            const float s0 = col_sum(hsum(sv0)), s1 = col_sum(hsum(R));
            if (act) lbrun = lsuf[chs + hi] + (top ? 0.0 : (double)__logf(s0) - (double)__logf(s1));
        }
        bool conflict = false;
        {
            const Tile tl = seg_tile(act, lo, hi - lo + 1);
            Plan pw = p;
            pw.nsub = (wave_max(tl.len) + SUB - 1) / SUB;
            f4 re;
            double le = 0.0;
            backward_body<3, KIND_WIN>(A, E, R, lbrun, 0.f, nullptr, (size_t)QP, out, nullptr, tl, m, seg, pw, eps, &re, nullptr, &le);
            if (act) { R = re; lbrun = le; }
        }
        // how far down a window may grow: to the top chunk of the nearest window below it that is walked at all
        int lob = 0;
        {
            const int top_act = act ? hi : -1;
            for (int i = 0; i < nwin; ++i) {
                const int v = __builtin_amdgcn_readlane(top_act, i);
                lob = (i < n) ? max(lob, v + 1) : lob;
            }
        }
        bool merged = !act;
        int ext = ext0, walked = act ? hi - lo + 1 : 0;
        while (true) {
            const bool chk = act && lo > 0;
            const f4 rsv = ld4(chk, rstart + (chs + lo) * QP);
            const f4 aw = ld4(chk, prefix + (chs + lo) * QP);
            const f4 ge = aw * R, gs = aw * rsv;
            const float i1 = __builtin_amdgcn_rcpf(col_sum(hsum(ge))), i2 = __builtin_amdgcn_rcpf(col_sum(hsum(gs)));
            float d = col_max(hmax(abs4(ge * i1 - gs * i2)));
            d = fmaxf(d, col_max(hmax(abs4(R - rsv))));
            if (act && !merged) merged = lo == 0 || d <= WIN_TOL;
            bool on = act && !merged && !conflict;
            int a = 0, nch = 0;
            if (on) {
                a = max(lob, lo - ext);
                if (a > lo - 1) { conflict = true; on = false; }
                nch = lo - a;
            }
            if (__builtin_amdgcn_ballot_w64(on) == 0ull) break;
            const Tile tl = seg_tile(on, a, nch);
            Plan pw = p;
            pw.nsub = (wave_max(tl.len) + SUB - 1) / SUB;
            f4 re;
            double le = 0.0;
            backward_body<3, KIND_WIN>(A, E, R, lbrun, 0.f, nullptr, (size_t)QP, out, nullptr, tl, m, seg, pw, eps, &re, nullptr, &le);
            if (on) { R = re; lbrun = le; lo = a; walked += nch; }
            ext *= 2;
        }
        bool good = __builtin_amdgcn_ballot_w64(valid && conflict) == 0ull;
        // what the rows below the window move by: the window's log scale at its lower end against the chunk scan's
        // (log beta of the last position below the window, both ways: the vectors agree up to scale there)
        double dlb = 0.0;
        {
            const bool dn = act && lo > 0;
            const f4 sv = ld4(dn, suffix + (chs + max(lo, 1) - 1) * QP);
            const float sr = col_sum(hsum(R)), ss = col_sum(hsum(sv));
            if (dn) dlb = (lbrun + (double)__logf(sr)) - (lsuf[chs + lo - 1] + (double)__logf(ss));
        }
        good = good && __builtin_amdgcn_ballot_w64(valid && !__builtin_isfinite(dlb)) == 0ull;   // (a chunk scan that broke down)
        if (valid && g == 0) {
            double *ws_ = wshift + (size_t)seq * WSH_STRIDE;
            ws_[n] = dlb;
            reinterpret_cast<int *>(ws_ + WIN_MAX)[n] = act ? lo : C;       // (inactive: above every chunk, shifts nothing)
        }
        int wsum = 0;
        for (int i = 0; i < nwin; ++i) wsum += __builtin_amdgcn_readlane(walked, i);
        if (lane == 0) {
            atomicAdd(wcnt + 3, wsum);
            if (!good) { flags[seq] = ROUTE_WHOLE; atomicAdd(wcnt + 1, 1); }
        }
    }
}

// log beta after the windows: every row of chunk c moves by the log-scale shifts of the windows that BEGIN above c
__global__ __launch_bounds__(256) void k_window_shift_logb(float *__restrict__ out, const int *__restrict__ wtab,
                                                           const int *__restrict__ wlist, const int *__restrict__ wcnt,
                                                           const int *__restrict__ flags, const double *__restrict__ wshift,
                                                           Plan p) {
    const int nlist = wcnt[0];
    const size_t rowsz = (size_t)p.q;
    for (int it = blockIdx.y; it < nlist; it += gridDim.y) {
        const int seq = wlist[it];
        if (flags[seq] != ROUTE_WINDOWS) continue;
        const int nwin = wtab[(size_t)seq * WIN_STRIDE];
        const double *d = wshift + (size_t)seq * WSH_STRIDE;
        const int *los = reinterpret_cast<const int *>(d + WIN_MAX);
        int top = 0;                                                 // nothing moves at or above the highest window's start
        for (int w = 0; w < nwin; ++w) top = (d[w] != 0.0 && los[w] > top) ? los[w] : top;
        float *o = out + (size_t)seq * p.L * rowsz;
        const size_t total = min((size_t)top * p.T, (size_t)p.L) * rowsz;
        for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
            const int c = (int)(i / (rowsz * p.T));
            double sh = 0.0;
            for (int w = 0; w < nwin; ++w) sh += los[w] > c ? d[w] : 0.0;
            o[i] += (float)sh;
        }
    }
}

// log alpha after the windows: every row of chunk c moves by the log-likelihood shifts of the windows that END before
// c (rows inside a window carry the chunk scan's value at the window's start already).  One block column per sequence
// of the window list; sequences that go on to the whole-sequence kernel are rewritten there.
__global__ __launch_bounds__(256) void k_window_shift_loga(float *__restrict__ out, const int *__restrict__ wtab,
                                                           const int *__restrict__ wlist, const int *__restrict__ wcnt,
                                                           const int *__restrict__ flags, const double *__restrict__ wshift,
                                                           Plan p) {
    const int nlist = wcnt[0];
    const size_t rowsz = (size_t)p.q;
    for (int it = blockIdx.y; it < nlist; it += gridDim.y) {
        const int seq = wlist[it];
        if (flags[seq] != ROUTE_WINDOWS) continue;
        const int nwin = wtab[(size_t)seq * WIN_STRIDE];
        const double *d = wshift + (size_t)seq * WSH_STRIDE;
        const int *his = reinterpret_cast<const int *>(d + WIN_MAX);
        const int c0 = his[0] + 1;                                   // nothing moves before the first window's end
        float *o = out + (size_t)seq * p.L * rowsz;
        const size_t first = (size_t)c0 * p.T * rowsz, total = (size_t)p.L * rowsz;
        for (size_t i = first + (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
            const int c = (int)(i / (rowsz * p.T));
            double sh = 0.0;
            for (int w = 0; w < nwin; ++w) sh += his[w] < c ? d[w] : 0.0;
            o[i] += (float)sh;
        }
    }
}

// HMM_POST_LOG_NO_LL (log gamma + loglik): the log-likelihood the windows corrected enters every position of the sequence
__global__ __launch_bounds__(256) void k_window_fixll(float *__restrict__ out, const int *__restrict__ wlist,
                                                      const int *__restrict__ wcnt, const int *__restrict__ flags,
                                                      const double *__restrict__ dfix, Plan p) {
    const int nlist = wcnt[0];
    const size_t per = (size_t)p.L * p.q;
    for (int it = blockIdx.y; it < nlist; it += gridDim.y) {
        const int seq = wlist[it];
        if (flags[seq] != ROUTE_WINDOWS) continue;
        const float d = (float)dfix[seq];
        if (d == 0.f) continue;
        float *o = out + (size_t)seq * per;
        for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < per; i += (size_t)gridDim.x * 256) o[i] += d;
    }
}

// The whole-sequence serial posterior in ONE launch (its waves exit at once when nothing is routed, so
// the common case pays one empty launch): forward pass writing checkpoints and the log-likelihood,
// then the backward pass of the same wave reading them back (same lanes, same addresses).
template <int MODE>
__global__ __launch_bounds__(256) void k_exact_posterior(const float *__restrict__ A, const float *__restrict__ pi,
                                                         const float *__restrict__ E, float *__restrict__ ckpt,
                                                         double *__restrict__ loglik, float *__restrict__ out,
                                                         Routing rt, Plan p, float eps, long long nwaves) {
    const long long wave = (long long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (wave >= nwaves) return;
    const int lane = threadIdx.x & 63, g = lane >> 4, n = lane & 15;
    int m; long long wc0;
    Tile tl = make_tile(E, p, wave, g, n, &m, &wc0);
    if (!route_tile<true>(tl, m, g, rt, eps)) return;
    __shared__ __attribute__((aligned(16))) float ostage[4 * OUT_SEG];
    float *seg = ostage + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) * OUT_SEG;
    float *ck = ckpt + ckpt_origin(tl, p, g, n);
    const double ll = forward_body<true, false, KIND_EXACT>(A, E, ld_state4(pi + (size_t)m * p.q, p.q, g), 0.0, ck,
                                                            ckpt_block(p), nullptr, tl, m, seg, p, eps);
    if (tl.valid && g == 0) loglik[tl.chain] = ll;
    __threadfence();
    backward_body<MODE, KIND_EXACT>(A, E, ones4(p.q, g), 0.0, (float)ll, ck, ckpt_block(p), out, nullptr, tl, m, seg, p, eps);
}

// k_exact_posterior<0> with the Decode output policy (hmm_posterior_decode) or ClassOut (hmm_class_posterior)
template <class DEC = Decode>
__global__ __launch_bounds__(256) void k_exact_decode(const float *__restrict__ A, const float *__restrict__ pi,
                                                      const float *__restrict__ E, float *__restrict__ ckpt,
                                                      double *__restrict__ loglik, Routing rt, Plan p, float eps,
                                                      long long nwaves, const DEC dec) {
    const long long wave = (long long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (wave >= nwaves) return;
    const int lane = threadIdx.x & 63, g = lane >> 4, n = lane & 15;
    int m; long long wc0;
    Tile tl = make_tile(E, p, wave, g, n, &m, &wc0);
    if (!route_tile<true>(tl, m, g, rt, eps)) return;
    __shared__ __attribute__((aligned(16))) float ostage[4 * OUT_SEG];
    float *seg = ostage + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) * OUT_SEG;
    float *ck = ckpt + ckpt_origin(tl, p, g, n);
    const double ll = forward_body<true, false, KIND_EXACT>(A, E, ld_state4(pi + (size_t)m * p.q, p.q, g), 0.0, ck,
                                                            ckpt_block(p), nullptr, tl, m, seg, p, eps);
    if (tl.valid && g == 0) loglik[tl.chain] = ll;
    __threadfence();
    backward_body<0, KIND_EXACT, false, SUB, DEC>(A, E, ones4(p.q, g), 0.0, 0.f, ck, ckpt_block(p), nullptr, nullptr, tl, m,
                                                  seg, p, eps, nullptr, nullptr, nullptr, dec);
}

// ------------------------------------------------------------------ small kernels

__global__ void k_copy_loglik(const double *__restrict__ src, double *__restrict__ dst, int n) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = src[i];
}

// (sum_b w*loglik, sum_b w) per model; one block per model, deterministic tree
__global__ __launch_bounds__(256) void k_loglik_partials(const double *__restrict__ ll, const float *__restrict__ w,
                                                         int b, double *__restrict__ partial) {
    __shared__ double s1[256], s2[256];
    const int m = blockIdx.x;
    double a = 0.0, c = 0.0;
    for (int i = threadIdx.x; i < b; i += 256) {
        double wi = w ? (double)w[(size_t)m * b + i] : 1.0;
        a += wi * ll[(size_t)m * b + i];
        c += wi;
    }
    s1[threadIdx.x] = a; s2[threadIdx.x] = c;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) { s1[threadIdx.x] += s1[threadIdx.x + s]; s2[threadIdx.x] += s2[threadIdx.x + s]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { partial[2 * m] = s1[0]; partial[2 * m + 1] = s2[0]; }
}

// ------------------------------------------------------------------ host side

#include "hmm_scan16.inc"

#include "hmm_largeq.inc"
#include "hmm_midq.inc"
#include "hmm_scan_rows.inc"
#include "hmm_scan_mid.inc"
#include "hmm_seqshard_mid.inc"
#include "hmm_wideq.inc"

// ---- the router: which path serves (op, k, b, L, q), the plans that path needs, the workspace it takes.  Every entry
// point below and hmm_workspace_bytes go through it, so they cannot disagree.
enum Path {
    PATH_S16,      // up to 16 states: the chunked scan of hmm_scan16.inc
    PATH_MID32,    // 17..32 states: the chunked scan of hmm_scan_mid.inc on 32-lane rows, one wave per sequence for the rest
    PATH_MID64,    // few long sequences of 33..64 states: the same on 64-lane rows
    PATH_MQ,       // up to 64 states otherwise: one wave per sequence (hmm_midq.inc)
    PATH_LQ        // above: one GEMM per step (hmm_largeq.inc)
};
struct Route {
    Path path;
    Plan p;            // S16, every operation but the posterior
    Groups G;          // S16, the posterior: one plan per batch group
    LqPlan lp;         // the other paths; MID*: the chunked scan's region (mp) follows it in the workspace
    MidPlan mp;
    size_t total;      // workspace bytes
};

static int make_route(int op, int k, int b, int L, int q, Route *r) {
    const int W = op != HMM_OP_VITERBI ? mid_width(k, b, L, q) : 0;
    r->path = q <= QP ? PATH_S16 : W == Q32 ? PATH_MID32 : W == Q64 ? PATH_MID64 : q <= MQ_MAX ? PATH_MQ : PATH_LQ;
    r->lp = LqPlan{};
    int rc;
    if (r->path == PATH_S16) {
        if (op == HMM_OP_POSTERIOR) {
            if ((rc = plan_groups(k, b, L, q, &r->G))) return rc;
            r->total = r->G.total;
        } else {
            if ((rc = make_plan(op, k, b, L, q, &r->p))) return rc;
            r->total = r->p.total;
        }
        return HMM_OK;
    }
    if ((rc = make_lqplan(k, b, L, q, &r->lp))) return rc;
    r->total = r->lp.total;
    if (W) {
        if ((rc = make_midplan(op, k, b, L, q, W, &r->mp))) return rc;
        r->total += r->mp.total;
    }
    return HMM_OK;
}

extern "C" {

const char *hmm_strerror(int code) {
    switch (code) {
        case HMM_OK: return "ok";
        case HMM_ERR_BAD_SHAPE: return "bad shape (k, b, L, q must be >= 1)";
        case HMM_ERR_Q_UNSUPPORTED: return "number of states not supported by this build (q <= 4096; Viterbi q <= 16)";
        case HMM_ERR_NULL_POINTER: return "null pointer";
        case HMM_ERR_WORKSPACE: return "workspace too small or not 256-byte aligned";
        case HMM_ERR_LAUNCH: return "HIP kernel launch failed";
        case HMM_ERR_BAD_ARGUMENT: return "bad argument";
        case HMM_ERR_NO_DEVICE: return "no HIP device";
        case HMM_ERR_NO_RCCL: return "ncclAllReduce not found: the host process has not loaded RCCL";
        default: return "unknown error";
    }
}

int hmm_abi_version(void) { return HMM_ENGINE_ABI_VERSION; }

int hmm_set_option(int option, int value) {
    if (option < 0 || option >= HMM_OPT_COUNT) return HMM_ERR_BAD_ARGUMENT;
    (void)opt(option);                                       // seeds the table on first use
    return g_opt[option].exchange(value);
}
int hmm_get_option(int option) {
    if (option < 0 || option >= HMM_OPT_COUNT) return HMM_ERR_BAD_ARGUMENT;
    return opt(option);
}
int hmm_max_states(void) { return HMM_LARGEQ_MAX; }
int hmm_scan_max_states(void) { return QP; }

int hmm_largeq_tile_cols(int b, int q) {
    if (b < 1 || q <= MQ_MAX || q > HMM_LARGEQ_MAX) return 0;
    return 16 * lq_tile_width(b, q);
}

int hmm_chunk_len(int k, int b, int L, int q) {
    if (q > QP) return q > HMM_LARGEQ_MAX ? HMM_ERR_Q_UNSUPPORTED : 0;     // 0: serial in time, no chunks
    Plan p;
    int rc = make_plan(HMM_OP_LOGLIK, k, b, L, q, &p);
    return rc ? rc : p.T;
}

int hmm_plan_capacity(int which) {
    switch (which) {
        case HMM_PLAN_CUS: return PLAN_CUS;
        case HMM_PLAN_FORWARD_BLOCKS:
        case HMM_PLAN_BACKWARD_BLOCKS: return PLAN_APPLY_BPC;
        case HMM_PLAN_REDUCE_BLOCKS: return PLAN_REDUCE_BPC;
        default: return HMM_ERR_BAD_ARGUMENT;
    }
}

int hmm_plan_capacity_device(int which) {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess) return HMM_ERR_NO_DEVICE;
    hipError_t e;
    switch (which) {
        case HMM_PLAN_CUS: e = hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev); break;
        case HMM_PLAN_FORWARD_BLOCKS:
            e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k_forward<true, false, false, false, HMM_POST_BLOCK>, 256, 0);
            break;
        case HMM_PLAN_BACKWARD_BLOCKS:
            e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k_backward<0, false, false, HMM_POST_BLOCK>, 256, 0);
            break;
        case HMM_PLAN_REDUCE_BLOCKS:
            e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k_reduce_sparse<TopoGene15>, 256, 0);
            break;
        default: return HMM_ERR_BAD_ARGUMENT;
    }
    return e == hipSuccess ? n : HMM_ERR_NO_DEVICE;
}

size_t hmm_workspace_bytes(int op, int k, int b, int L, int q) {
    Route r;
    return make_route(op, k, b, L, q, &r) ? 0 : r.total;
}

int hmm_forward(const float *A, const float *pi, const float *E, int k, int b, int L, int q, float eps,
                float *log_alpha, double *loglik, void *workspace, size_t workspace_bytes, void *stream) {
    Route r;
    int rc = make_route(log_alpha ? HMM_OP_FORWARD : HMM_OP_LOGLIK, k, b, L, q, &r);
    if (rc) return rc;
    if (!A || !pi || !E || !loglik) return HMM_ERR_NULL_POINTER;
    if ((rc = check_eps(eps))) return rc;
    if ((rc = check_ws(r.total, workspace, workspace_bytes))) return rc;
    char *ws = (char *)workspace;
    hipStream_t st = (hipStream_t)stream;
    char *wm = ws + r.lp.total;                              // MID*: the chunked scan's region
    double *ll = ws_at<double>(ws, r.lp.o_ll);
    const int *need = nullptr;
    MqSp *sp = ws_at<MqSp>(ws, r.lp.o_sp);
    switch (r.path) {
        case PATH_S16: return s16_forward(A, pi, E, r.p, eps, log_alpha, loglik, ws, st);
        case PATH_MID32:
        case PATH_MID64:
            // chunk operators + chunk scan (+ the forward apply kernel for log alpha) for the models the chunked path
            // serves (decided on the device), one wave per sequence for the others
            if (log_alpha)
                (r.path == PATH_MID32 ? scan_forward<Scan32> : scan_forward<Scan64>)(A, pi, E, r.mp, eps, log_alpha, wm, st);
            else
                (r.path == PATH_MID32 ? scan_loglik<Scan32> : scan_loglik<Scan64>)(A, pi, E, r.mp, eps, wm, st);
            ll = WsMid(r.mp, wm).loglik;
            need = WsMid(r.mp, wm).need;
            [[fallthrough]];
        case PATH_MQ:                                        // one wave per sequence, no launches per step
            mq_forward(A, pi, E, k, b, L, q, eps, nullptr, log_alpha, ll, st, need, sp);
            break;
        case PATH_LQ: lq_forward(A, pi, E, r.lp, eps, ws, log_alpha, st); break;
    }
    launch(k_copy_loglik, dim3((r.lp.NB + 255) / 256), dim3(256), 0, st, ll, loglik, r.lp.NB);
    return check_launch();
}

int hmm_backward(const float *A, const float *E, int k, int b, int L, int q, float eps, float *log_beta,
                 void *workspace, size_t workspace_bytes, void *stream) {
    Route r;
    int rc = make_route(HMM_OP_BACKWARD, k, b, L, q, &r);
    if (rc) return rc;
    if (!A || !E || !log_beta) return HMM_ERR_NULL_POINTER;
    if ((rc = check_eps(eps))) return rc;
    if ((rc = check_ws(r.total, workspace, workspace_bytes))) return rc;
    char *ws = (char *)workspace;
    hipStream_t st = (hipStream_t)stream;
    char *wm = ws + r.lp.total;                              // MID*: the chunked scan's region
    const int *need = nullptr;
    MqSp *sp = ws_at<MqSp>(ws, r.lp.o_sp);
    switch (r.path) {
        case PATH_S16: return s16_backward(A, E, r.p, eps, log_beta, ws, st);
        case PATH_MID32:
        case PATH_MID64:
            (r.path == PATH_MID32 ? scan_backward<Scan32> : scan_backward<Scan64>)(A, E, r.mp, eps, log_beta, wm, st);
            need = WsMid(r.mp, wm).need;
            [[fallthrough]];
        case PATH_MQ: mq_backward(A, E, k, b, L, q, eps, log_beta, nullptr, 3, st, need, sp); break;
        case PATH_LQ: lq_backward(A, E, r.lp, eps, ws, log_beta, st); break;
    }
    return check_launch();
}

static int posterior_impl(const float *A, const float *pi, const float *E, int k, int b, int L, int q, float eps,
                          int mode, float *out, double *loglik, void *workspace, size_t workspace_bytes,
                          void *stream, Profile *pr) {
    Route r;
    int rc = make_route(HMM_OP_POSTERIOR, k, b, L, q, &r);
    if (rc) return rc;
    if (!A || !pi || !E || !out) return HMM_ERR_NULL_POINTER;
    if (mode < HMM_POST_PROB || mode > HMM_POST_LOG_NO_LL) return HMM_ERR_BAD_ARGUMENT;
    if ((rc = check_eps(eps))) return rc;
    if ((rc = check_ws(r.total, workspace, workspace_bytes))) return rc;
    char *ws = (char *)workspace;
    hipStream_t st = (hipStream_t)stream;
    char *wm = ws + r.lp.total;                              // MID*: the chunked scan's region
    double *ll = ws_at<double>(ws, r.lp.o_ll);
    const int *need = nullptr;
    MqSp *sp = ws_at<MqSp>(ws, r.lp.o_sp);
    switch (r.path) {
        case PATH_S16: return s16_posterior(A, pi, E, r.G, eps, mode, out, loglik, ws, st, pr);
        case PATH_MID32:
        case PATH_MID64:
            // the chunked scan for the models it serves, the serial kernels for the rest and for the sequences the
            // certificate flags (all decided on the device)
            (r.path == PATH_MID32 ? scan_posterior<Scan32> : scan_posterior<Scan64>)(A, pi, E, r.mp, eps, mode, out, wm,
                                                                                     st, nullptr);
            ll = WsMid(r.mp, wm).loglik;
            need = WsMid(r.mp, wm).need;
            [[fallthrough]];
        case PATH_MQ:
            if (mode != HMM_POST_LOG_NO_LL && L >= 2) {      // forward and backward waves side by side, meeting in the middle
                mq_posterior2(A, pi, E, k, b, L, q, eps, out, ll, mode, st, need, sp);
            } else {
                mq_forward(A, pi, E, k, b, L, q, eps, out, nullptr, ll, st, need, sp);   // alpha_hat parked in `out`
                mq_backward(A, E, k, b, L, q, eps, out, ll, mode, st, need, sp);
            }
            break;
        case PATH_LQ: {
            hipStream_t *hs = helper_streams();               // the two recursions side by side (lq_posterior)
            lq_posterior(A, pi, E, r.lp, eps, ws, out, mode, st, hs ? hs[0] : nullptr);
            break;
        }
    }
    if (loglik) launch(k_copy_loglik, dim3((r.lp.NB + 255) / 256), dim3(256), 0, st, ll, loglik, r.lp.NB);
    return check_launch();
}

int hmm_posterior(const float *A, const float *pi, const float *E, int k, int b, int L, int q, float eps,
                  int mode, float *out, double *loglik, void *workspace, size_t workspace_bytes, void *stream) {
    return posterior_impl(A, pi, E, k, b, L, q, eps, mode, out, loglik, workspace, workspace_bytes, stream, nullptr);
}

int hmm_posterior_decode_max_states(void) { return QP; }

int hmm_posterior_decode(const float *A, const float *pi, const float *E, int k, int b, int L, int q, float eps,
                         const int *state_class, int num_classes, unsigned char *label, float *conf, double *loglik,
                         void *workspace, size_t workspace_bytes, void *stream) {
    if (k < 1 || b < 1 || L < 1 || q < 1) return HMM_ERR_BAD_SHAPE;
    if (q > QP) return HMM_ERR_Q_UNSUPPORTED;
    Route r;
    int rc = make_route(HMM_OP_POSTERIOR, k, b, L, q, &r);
    if (rc) return rc;
    if (!A || !pi || !E || !label || !workspace) return HMM_ERR_NULL_POINTER;
    if (num_classes < 1 || num_classes > QP || (!state_class && num_classes != q)) return HMM_ERR_BAD_ARGUMENT;
    if ((rc = check_eps(eps))) return rc;
    Decode dec{};
    dec.label = label; dec.conf = conf; dec.ncls = state_class ? num_classes : 0;
    for (int s = 0; s < q && state_class; ++s) {               // the table is read here, once, and travels by value
        if (state_class[s] < 0 || state_class[s] >= num_classes) return HMM_ERR_BAD_ARGUMENT;
        dec.w[state_class[s]][s] = 1.f;
    }
    if ((rc = check_ws(r.total, workspace, workspace_bytes))) return rc;
    return s16_posterior(A, pi, E, r.G, eps, HMM_POST_PROB, nullptr, loglik, (char *)workspace, (hipStream_t)stream,
                         nullptr, &dec);
}

int hmm_posterior_decode_mid_max_states(void) { return MQ_MAX; }

// hmm_posterior's workspace, then the parking region of the serial walk: k b L q floats, addressed like `out`
static size_t decode_mid_park(const Route &r) { return align_up(r.total); }

size_t hmm_posterior_decode_mid_workspace_bytes(int k, int b, int L, int q) {
    Route r;
    if (q <= QP || q > MQ_MAX || make_route(HMM_OP_POSTERIOR, k, b, L, q, &r)) return 0;
    return decode_mid_park(r) + (size_t)k * b * L * q * sizeof(float);
}

int hmm_posterior_decode_mid(const float *A, const float *pi, const float *E, int k, int b, int L, int q, float eps,
                             const int *state_class, int num_classes, unsigned char *label, float *conf,
                             double *loglik, void *workspace, size_t workspace_bytes, void *stream) {
    if (k < 1 || b < 1 || L < 1 || q < 1) return HMM_ERR_BAD_SHAPE;
    if (q <= QP || q > MQ_MAX) return HMM_ERR_Q_UNSUPPORTED;
    Route r;
    int rc = make_route(HMM_OP_POSTERIOR, k, b, L, q, &r);
    if (rc) return rc;
    if (!A || !pi || !E || !label || !workspace) return HMM_ERR_NULL_POINTER;
    if (num_classes < 1 || (state_class ? num_classes > QP : num_classes != q)) return HMM_ERR_BAD_ARGUMENT;
    if ((rc = check_eps(eps))) return rc;
    DecodeMid dec{};
    dec.label = label; dec.conf = conf; dec.ncls = state_class ? num_classes : 0;
    for (int s = 0; s < q && state_class; ++s) {               // the table is read here, once, and travels by value
        if (state_class[s] < 0 || state_class[s] >= num_classes) return HMM_ERR_BAD_ARGUMENT;
        dec.mask[state_class[s]] |= 1ull << s;
    }
    const size_t o_park = decode_mid_park(r);
    if ((rc = check_ws(o_park + (size_t)k * b * L * q * sizeof(float), workspace, workspace_bytes))) return rc;
    char *ws = (char *)workspace;
    hipStream_t st = (hipStream_t)stream;
    char *wm = ws + r.lp.total;                              // MID*: the chunked scan's region
    double *ll = ws_at<double>(ws, r.lp.o_ll);
    const int *need = nullptr;
    if (r.path != PATH_MQ) {
        (r.path == PATH_MID32 ? scan_posterior<Scan32> : scan_posterior<Scan64>)(A, pi, E, r.mp, eps, HMM_POST_PROB,
                                                                                 nullptr, wm, st, &dec);
        ll = WsMid(r.mp, wm).loglik;
        need = WsMid(r.mp, wm).need;
    }
    mq_posterior2_decode(A, pi, E, k, b, L, q, eps, ws_at<float>(ws, o_park), ll, dec, st, need,
                         ws_at<MqSp>(ws, r.lp.o_sp));
    if (loglik) launch(k_copy_loglik, dim3((r.lp.NB + 255) / 256), dim3(256), 0, st, ll, loglik, r.lp.NB);
    return check_launch();
}

// one device counter -> the host, added to *sum
static int read_counter(const int *src, long long *sum) {
    int v = 0;
    if (hipMemcpy(&v, src, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return HMM_ERR_LAUNCH;
    *sum += v;
    return HMM_OK;
}

long long hmm_exact_count(int op, int k, int b, int L, int q, const void *workspace, size_t workspace_bytes) {
    Route r;
    int rc = make_route(op, k, b, L, q, &r);
    if (r.path == PATH_MQ || r.path == PATH_LQ) return 0;    // the serial-in-time paths are exact throughout
    if (rc && r.path != PATH_S16) return rc;
    if (!workspace) return HMM_ERR_NULL_POINTER;
    if (rc) return rc;
    if (workspace_bytes < r.total) return HMM_ERR_WORKSPACE;
    long long total = 0;
    if (r.path != PATH_S16)                                  // sequences of the last call that the one-wave-per-sequence kernels served
        rc = read_counter(WsMid(r.mp, (const char *)workspace + r.lp.total).nex, &total);
    else if (op != HMM_OP_POSTERIOR)
        rc = read_counter(Ws16(r.p, workspace).nexact, &total);
    else
        for (int g = 0; g < r.G.n && rc == HMM_OK; ++g)
            rc = read_counter(Ws16(r.G.plan[g], (const char *)workspace + r.G.off[g]).nexact, &total);
    return rc ? rc : total;
}

int hmm_exact_detail(int k, int b, int L, int q, const void *workspace, size_t workspace_bytes, long long *detail) {
    return hmm_exact_detail_op(HMM_OP_POSTERIOR, k, b, L, q, workspace, workspace_bytes, detail);
}

int hmm_exact_detail_op(int op, int k, int b, int L, int q, const void *workspace, size_t workspace_bytes,
                        long long *detail) {
    if (!workspace || !detail) return HMM_ERR_NULL_POINTER;
    if (q > QP) return HMM_ERR_Q_UNSUPPORTED;
    // the routing counters of the plan at `off` in the workspace, added to detail[]
    auto read = [&](const Plan &p, size_t off) -> int {
        if (workspace_bytes < off + p.total) return HMM_ERR_WORKSPACE;
        int nx = 0, wc[4] = {0, 0, 0, 0};
        const Ws16 w(p, (const char *)workspace + off);
        if (hipMemcpy(&nx, w.nexact, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(wc, w.wcnt, sizeof(wc), hipMemcpyDeviceToHost) != hipSuccess)
            return HMM_ERR_LAUNCH;
        detail[0] += nx; detail[1] += wc[0]; detail[2] += wc[2]; detail[3] += wc[1]; detail[4] += wc[3];
        return HMM_OK;
    };
    int rc;
    if (op == HMM_OP_POSTERIOR) {                            // one plan per group of sequences
        Groups G;
        if ((rc = plan_groups(k, b, L, q, &G))) return rc;
        for (int i = 0; i < 5; ++i) detail[i] = 0;
        for (int g = 0; g < G.n; ++g)
            if ((rc = read(G.plan[g], G.off[g]))) return rc;
        return HMM_OK;
    }
    if (op != HMM_OP_LOGLIK && op != HMM_OP_FORWARD && op != HMM_OP_BACKWARD) return HMM_ERR_BAD_ARGUMENT;
    Plan p;
    if ((rc = make_plan(op, k, b, L, q, &p))) return rc;
    if (workspace_bytes < p.total) return HMM_ERR_WORKSPACE;
    for (int i = 0; i < 5; ++i) detail[i] = 0;
    return read(p, 0);
}

int hmm_window_table(int op, int k, int b, int L, int q, const void *workspace, size_t workspace_bytes, int seq,
                     int *table, double *shifts, float *psi, int npsi) {
    if (!workspace || !table) return HMM_ERR_NULL_POINTER;
    if (q > QP) return HMM_ERR_Q_UNSUPPORTED;
    Plan p;
    int rc = make_plan(op, k, b, L, q, &p);
    if (rc) return rc;
    if (workspace_bytes < p.total || seq < 0 || seq >= p.NB) return HMM_ERR_WORKSPACE;
    const Ws16 w(p, workspace);
    if (hipMemcpy(table, w.wtab + (size_t)seq * WIN_STRIDE, WIN_STRIDE * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess)
        return HMM_ERR_LAUNCH;
    if (shifts && (op == HMM_OP_FORWARD || op == HMM_OP_BACKWARD) &&
        hipMemcpy(shifts, w.wshift + (size_t)seq * WSH_STRIDE, WSH_STRIDE * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
        return HMM_ERR_LAUNCH;
    if (psi && npsi > 0) {
        const int n = npsi < p.C ? npsi : p.C;
        if (hipMemcpy(psi, w.phi + (size_t)seq * p.C, (size_t)n * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess)
            return HMM_ERR_LAUNCH;
    }
    return p.C;
}

void *hmm_profile_create(void) { return new Profile(); }

void hmm_profile_destroy(void *profile) {
    Profile *pr = (Profile *)profile;
    if (!pr) return;
    for (auto &s : pr->spans) { (void)hipEventDestroy(s.a); (void)hipEventDestroy(s.b); }
    delete pr;
}

int hmm_posterior_profiled(const float *A, const float *pi, const float *E, int k, int b, int L, int q, float eps,
                           int mode, float *out, double *loglik, void *workspace, size_t workspace_bytes,
                           void *stream, void *profile) {
    return posterior_impl(A, pi, E, k, b, L, q, eps, mode, out, loglik, workspace, workspace_bytes, stream,
                          (Profile *)profile);
}

int hmm_profile_read(void *profile, double *ms, long long *launches) {
    Profile *pr = (Profile *)profile;
    if (!pr || !ms || !launches) return HMM_ERR_NULL_POINTER;
    for (int i = 0; i < HMM_KERNEL_COUNT; ++i) { ms[i] = 0.0; launches[i] = 0; }
    for (auto &s : pr->spans) {
        if (hipEventSynchronize(s.b) != hipSuccess) return HMM_ERR_LAUNCH;
        float t = 0.f;
        if (hipEventElapsedTime(&t, s.a, s.b) != hipSuccess) return HMM_ERR_LAUNCH;
        ms[s.kernel] += t;
        launches[s.kernel] += 1;
        (void)hipEventDestroy(s.a); (void)hipEventDestroy(s.b);
    }
    pr->spans.clear();
    return HMM_OK;
}

// The one collective of the path for hosts without torch.distributed: all-reduce(sum) of the (k,2)
// partials over an RCCL communicator the HOST created.  RCCL is not linked: ncclAllReduce is looked up
// among the libraries the process has already loaded (the host's own RCCL, the one its communicator
// belongs to), so the engine never brings a second copy of the library into the process.
#include <dlfcn.h>
int hmm_loglik_allreduce(void *comm, double *partial, int k, void *stream) {
    typedef int (*allreduce_fn)(const void *, void *, size_t, int, int, void *, hipStream_t);
    if (k < 1) return HMM_ERR_BAD_SHAPE;
    if (!comm || !partial) return HMM_ERR_NULL_POINTER;
    static std::atomic<allreduce_fn> cached{nullptr};
    allreduce_fn fn = cached.load();
    if (!fn) {
        fn = (allreduce_fn)dlsym(RTLD_DEFAULT, "ncclAllReduce");
        if (!fn) {
            // a host that loaded RCCL without global symbol visibility (dlopen(..., RTLD_LOCAL), as Python extension
            // modules do): ask for the handle of the copy that is ALREADY in the process — RTLD_NOLOAD never loads one
            static const char *names[] = {"librccl.so", "librccl.so.1", "libnccl.so", "libnccl.so.2"};
            for (const char *nm : names) {
                void *h = dlopen(nm, RTLD_NOLOAD | RTLD_NOW);
                if (h && (fn = (allreduce_fn)dlsym(h, "ncclAllReduce"))) break;
            }
        }
        if (!fn) return HMM_ERR_NO_RCCL;
        cached.store(fn);
    }
    const int ncclFloat64 = 8, ncclSum = 0;                  // rccl.h: ncclDataType_t, ncclRedOp_t
    return fn(partial, partial, (size_t)2 * k, ncclFloat64, ncclSum, comm, (hipStream_t)stream) == 0 ? HMM_OK
                                                                                                     : HMM_ERR_LAUNCH;
}

int hmm_loglik_partials(const double *loglik, const float *weights, int k, int b, double *partial, void *stream) {
    if (k < 1 || b < 1) return HMM_ERR_BAD_SHAPE;
    if (!loglik || !partial) return HMM_ERR_NULL_POINTER;
    launch(k_loglik_partials, dim3(k), dim3(256), 0, (hipStream_t)stream, loglik, weights, b, partial);
    return check_launch();
}

}  // extern "C"

#include "hmm_seqshard.inc"
#include "hmm_viterbi.inc"
#include "hmm_seqshard_viterbi.inc"
#include "hmm_viterbi_scan.inc"
#include "hmm_seqshard_vscan.inc"
#include "hmm_viterbi_large.inc"
#include "hmm_emitter.inc"
#include "hmm_emitter_grad.inc"
#include "hmm_emitter_mvn.inc"
#include "hmm_emitter_mvn_grad.inc"
#include "hmm_emitter_mvn_wide.inc"
#include "hmm_emitter_mvn_grad_wide.inc"
#include "hmm_emitter_nuc.inc"
#include "hmm_grad.inc"
#include "hmm_postgrad.inc"
#include "hmm_grad_scan.inc"
#include "hmm_postgrad_scan.inc"
#include "hmm_grad_large.inc"
#include "hmm_gradwq.inc"
#include "hmm_postgrad_large.inc"
#include "hmm_postgradwq.inc"
#include "hmm_class_posterior.inc"
