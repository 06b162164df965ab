// hmm_emitter.inc — fused producer of the emission tensor for the gene-prediction models,
// included by hmm_engine.hip.  Replaces GenePredHMMEmitter.forward
// (hmm_layer/gene_pred_hmm_emitter.py:231-277 over SimpleGenePredHMMEmitter.forward :93-121 and
// kmer.make_k_mers, hmm_layer/kmer.py:3-47) for inference: class probabilities (s per position)
// and one-hot nucleotides (A,C,G,T,N) in, E (b,L,q) out.  The reference materialises two (b,L,64)
// 3-mer tensors and a (b,L,2,q) product on the way; here neither exists.
//
//   emit[j] = sum_s x[s] * B[state_row[j]][s]                                (:113-116)
//   left / right 3-mer distribution of position t from the nucleotides at t..t+2 / t-2..t, N spread
//   uniformly, uniform padding over the sequence border                     (kmer.py:19-33)
//   cod[j]  = state_codon[j] < 0 ? free_value
//                                : <left3, T[0][c]> * <right3, T[1][c]>      (:247-258)
//   E[j]    = emit[j] * (cod[j] + add)                                       (:260-262)
// 3-mer class index: left  = 16*nuc(t+1) + 4*nuc(t+2) + nuc(t),
//                    right = 16*nuc(t-1) + 4*nuc(t-2) + nuc(t)              (kmer.py:36-46).
//
// Shape of the kernel.  A wave owns runs of EM_RUN consecutive positions and walks them 16 at a
// time.  emit for a 16-position x 16-state tile is X (16 x s) times Bexp^T (s x 16): four
// v_mfma_f32_16x16x4_f32 with the input rows loaded straight into the A-operand layout (lane
// (g, m) holds classes 4g..4g+3 of position m: one 16-byte load per lane, every element of x read
// once) and the expanded emission kernel constant in the B-operand registers.  The D layout puts
// state n of positions 4g..4g+3 in lane (g, n).
// Nucleotides are one-hot almost everywhere, so a window is described by bits: every lane
// classifies its position into a 3-bit code (A,C,G,T -> 0..3, exact N -> 4; anything else is
// "soft"), a DPP OR-reduction packs the 16 codes of the tile into one wave-uniform 48-bit word,
// and the words of the previous, current and next tile form a 20-position window (60 bits).  The
// 9 bits starting at 3 x (window offset) ARE the index into a per-(side, table row) LDS table that
// holds, for any combination of A/C/G/T/N in the three slots, the 3-mer factor (N slots summed out
// with their uniform weight): per lane one 64-bit shift per tile, then a bit-field extract and
// one lookup per side and position — no arithmetic on the one-hot floats.  Tiles whose window
// holds a soft distribution or a sequence border (a wave-uniform test) take a generic path that
// evaluates the reference's 64-term product-sum from memory where needed.
//
// The file holds both forwards — hmm_gene_emissions (q <= 64, rows <= 32) and, further down, hmm_gene_emissions_wide
// (up to 256 states and rows) — and the pieces all four gene kernels share (the two backwards are in
// hmm_emitter_grad.inc): the window tables and code words (em_build_tables, em_classify), the scale of one tile
// (em_scale_tile), the run walker (em_walk), the flat flush of a contiguous tile (em_flush_flat), the clamped reads of
// state_row / state_codon (em_row, em_codon), and the host side's argument check, run length and grid.
//
// Compiler figures (gfx950, hipcc -O3; no instantiation uses scratch): k_gene_emissions<1, 1, FAST> 119 VGPRs,
// <1, 1, false> 110, <4, 2, false> 176; k_gene_emissions_wide 197.

#define EM_MAXQ 64          // states
#define EM_MAXS 32          // classes
#define EM_MAXC 16          // 3-mer table rows per side
#define EM_MAXR 32          // emission-kernel rows
#define EM_RUN 1024         // positions per wave run
#define EM_THREADS 512      // 8 waves share one copy of the window tables

// generic window (soft nucleotides and/or sequence border): the reference's product-sum, slot k of
// side 0 = position t+k, of side 1 = position t-2+k; table rows are read at their one-hot indices
__device__ __forceinline__ float em_slow_factor(const float *__restrict__ x, long long pos, int t, int L, int s, int w,
                                                const float *TL, const float *TR, float n_mass) {
    float prod = 1.f;
#pragma unroll
    for (int side = 0; side < 2; ++side) {
        const float *T = side ? TR : TL;
        const float nm = side ? n_mass : 1.f;
        float q0[4], q1[4], q2[4];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int d = side ? k - 2 : k;
            const int tt = t + d;
            float v[4] = {0.25f, 0.25f, 0.25f, 0.25f};
            if (tt >= 0 && tt < L) {
                const float *r = x + (pos + d) * w + s;
                const float wn = (r[4] == 1.f) ? 0.25f * nm : 0.f;
                v[0] = r[0] + wn; v[1] = r[1] + wn; v[2] = r[2] + wn; v[3] = r[3] + wn;
            }
#pragma unroll
            for (int a = 0; a < 4; ++a) { if (k == 0) q0[a] = v[a]; else if (k == 1) q1[a] = v[a]; else q2[a] = v[a]; }
        }
        // outer loops stay rolled (run-time index -> compare-select): this path is rare and must not
        // set the kernel's register budget
        float acc = 0.f;
#pragma unroll 1
        for (int a2 = 0; a2 < 4; ++a2) {
            const float v2 = a2 == 0 ? q2[0] : a2 == 1 ? q2[1] : a2 == 2 ? q2[2] : q2[3];
#pragma unroll 1
            for (int a1 = 0; a1 < 4; ++a1) {
                const float v12 = v2 * (a1 == 0 ? q1[0] : a1 == 1 ? q1[1] : a1 == 2 ? q1[2] : q1[3]);
#pragma unroll
                for (int a0 = 0; a0 < 4; ++a0) acc = fmaf(q0[a0] * v12, T[a0 | (a1 << 3) | (a2 << 6)], acc);
            }
        }
        prod *= acc;
    }
    return prod;
}

// ---- pieces shared by the four gene kernels

struct EmNuc { f4 nv; float nN; };                           // the five nucleotide floats of one position
struct EmCodes { unsigned long long v; unsigned soft; };     // 16 x 3-bit codes; positions holding a soft distribution

// the window tables: index = code(slot 0) | code(slot 1) << 3 | code(slot 2) << 6
__device__ __forceinline__ void em_build_tables(float *T9, const float *__restrict__ codon, int nc, float n_mass, int tid) {
    for (int e = tid; e < 2 * nc * 512; e += EM_THREADS) {
        const int idx = e & 511, sr = e >> 9;
        const int side = sr >= nc ? 1 : 0, c = sr - side * nc;
        const int c0 = idx & 7, c1 = (idx >> 3) & 7, c2 = (idx >> 6) & 7;
        float val = 0.f;
        if (c0 <= 4 && c1 <= 4 && c2 <= 4) {
            const float *T = codon + (size_t)(side * nc + c) * 64;
            const float wn = side ? 0.25f * n_mass : 0.25f;           // weight of one class of an N slot
            const int l0 = c0 < 4 ? c0 : 0, h0 = c0 < 4 ? c0 : 3;
            const int l1 = c1 < 4 ? c1 : 0, h1 = c1 < 4 ? c1 : 3;
            const int l2 = c2 < 4 ? c2 : 0, h2 = c2 < 4 ? c2 : 3;
            float acc = 0.f;
            for (int a0 = l0; a0 <= h0; ++a0)
                for (int a1 = l1; a1 <= h1; ++a1)
                    for (int a2 = l2; a2 <= h2; ++a2)
                        acc += T[side ? 16 * a1 + 4 * a0 + a2 : 16 * a1 + 4 * a2 + a0];
            val = acc * (c0 == 4 ? wn : 1.f) * (c1 == 4 ? wn : 1.f) * (c2 == 4 ? wn : 1.f);
        }
        T9[e] = val;
    }
}

__device__ __forceinline__ EmNuc em_load_nuc(const float *xr, int s) {
    EmNuc nu;
    nu.nv = *reinterpret_cast<const f4u *>(xr + s);
    nu.nN = xr[s + 4];
    return nu;
}

// lane (g, n) holds the nucleotides of position n of the tile -> the tile's wave-uniform code word
__device__ __forceinline__ EmCodes em_classify(const EmNuc &rw, int n) {
    const f4 nv = rw.nv;
    const bool isN = rw.nN == 1.f;                  // the reference counts N only when the flag is exactly 1
    const float sum = (nv.x + nv.y) + (nv.z + nv.w);
    const bool hot = !isN && sum == 1.f && (nv.x == 1.f || nv.y == 1.f || nv.z == 1.f || nv.w == 1.f);
    const bool exactN = isN && sum == 0.f;
    const int code = hot ? (nv.y == 1.f ? 1 : nv.z == 1.f ? 2 : nv.w == 1.f ? 3 : 0) : 4;
    // pack: positions 0..9 in one word, 10..15 in the other, OR over the 16 lanes of the row
    int lo = n < 10 ? code << (3 * n) : 0, hi = n < 10 ? 0 : code << (3 * (n - 10));
    auto bor = [](int a, int b) { return a | b; };
    lo = row_allreduce_i(lo, bor);
    hi = row_allreduce_i(hi, bor);
    EmCodes cd;
    cd.v = (unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane(lo) |
           ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane(hi) << 30);
    cd.soft = (unsigned)__ballot(!(hot || exactN)) & 0xFFFFu;
    return cd;
}

// One tile in the D layout (lane (g, n): state 16 nt + n at positions 4g..4g+3 of the tile starting at
// P, tb = P's position in its sequence): stage[pl * stride + j] = D[nt][r] * (cod[pl][j] + add) for every
// position below npos and state below q; other entries of the stage are left as they are.  The forward
// passes emit and its output stage (stride q), the backward dE and its H stage.
template <int NT>
__device__ __forceinline__ void em_scale_tile(const f4 (&D)[NT], float *stage, int stride, const int (&cj)[NT], int q,
                                              const float *T9, int ncp, const EmCodes &prev, const EmCodes &cur,
                                              const EmCodes &nxt, int tb, int L, long long P, long long npos, int g, int n,
                                              const float *__restrict__ x, int s, int w, float free_value, float add,
                                              float n_mass) {
    // 20-position window, 3 bits each: field p <-> position P - 2 + p
    const unsigned long long Wv = (prev.v >> 42) | (cur.v << 6) | (nxt.v << 54);
    const unsigned Ws = (prev.soft >> 14) | (cur.soft << 2) | (nxt.soft << 18);
    // this lane's positions 4g..4g+3 see fields 4g..4g+7: 24 bits
    const unsigned u = (unsigned)(Wv >> (12 * g));
    const bool plain = Ws == 0u && tb >= 2 && tb + 18 <= L && P + 16 <= npos;     // wave-uniform
    if (__builtin_expect(plain, 1)) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int j = 16 * nt + n;
            if (j >= q) continue;
            const int c = cj[nt];
            const float *TL = T9 + (c >= 0 ? c : 0) * 512, *TR = TL + ncp * 512;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float f = TL[(u >> (3 * r + 6)) & 511u] * TR[(u >> (3 * r)) & 511u];
                stage[(4 * g + r) * stride + j] = D[nt][r] * ((c >= 0 ? f : free_value) + add);
            }
        }
    } else {
        // a soft distribution, a sequence border or the end of the tensor inside the window:
        // per output, table lookup or the generic product-sum
        unsigned slowmask = 0;                      // bit 4 nt + r: that output needs the generic path
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int pl = 4 * g + r;
            const long long pos = P + pl;
            int t = tb + pl;
            if (t >= L) t %= L;
            const bool slow = ((Ws >> pl) & 0x1Fu) != 0u || t < 2 || t >= L - 2;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const int j = 16 * nt + n;
                const int c = cj[nt];
                float cod = free_value;
                if (c >= 0) cod = T9[c * 512 + ((u >> (3 * r + 6)) & 511u)] * T9[(ncp + c) * 512 + ((u >> (3 * r)) & 511u)];
                const bool ok = pos < npos && j < q;
                if (ok && c >= 0 && slow) slowmask |= 1u << (4 * nt + r);
                else if (ok) stage[pl * stride + j] = D[nt][r] * (cod + add);
            }
        }
        if (__ballot(slowmask != 0u) != 0ull) {
            // one copy of the generic code, walked with run-time indices (the tile values are
            // picked by compare-select)
#pragma unroll 1
            for (int o = 0; o < 4 * NT; ++o) {
                if (!((slowmask >> o) & 1u)) continue;
                const int nt = o >> 2, r = o & 3;
                float d = 0.f;
                int c = -1;
#pragma unroll
                for (int a = 0; a < NT; ++a) {
                    const float v = r == 0 ? D[a][0] : r == 1 ? D[a][1] : r == 2 ? D[a][2] : D[a][3];
                    d = a == nt ? v : d;
                    c = a == nt ? cj[a] : c;
                }
                const int pl = 4 * g + r;
                const long long pos = P + pl;
                int t = tb + pl;
                if (t >= L) t %= L;
                const float cod = em_slow_factor(x, pos, t, L, s, w, T9 + (size_t)c * 512,
                                                 T9 + (size_t)(ncp + c) * 512, n_mass);
                stage[pl * stride + 16 * nt + n] = d * (cod + add);
            }
        }
    }
}

// state -> emission-kernel row / 3-mer table row, clamped into the tables: an entry out of range reads a defined row
__device__ __forceinline__ int em_row(const int *__restrict__ state_row, int j, int rows) {
    const int r = state_row[j];
    return r < 0 ? 0 : (r >= rows ? rows - 1 : r);
}
__device__ __forceinline__ int em_codon(const int *__restrict__ state_codon, int j, int nc) {
    const int c = state_codon[j];
    return c < nc ? c : nc - 1;                                   // (nc = 0: every state is free)
}

// One tile of a run as the walker hands it to a kernel's body: P = its first position, tb = P's position in its
// sequence, the code words of the tile before, the tile and the tile after, and (forwards, KT > 0) the tile's class
// columns in the A-operand layout.
template <int KT>
struct EmTile { long long P; int tb; EmCodes prev, cur, nxt; f4 xa[KT > 0 ? KT : 1]; };

// The run walker of all four gene kernels.  Wave `tid >> 6` of workgroup blockIdx.x owns the runs wave0, wave0 + nwaves,
// .. of run_len consecutive positions and walks each 16 positions at a time: on_run(P0) once per run, then
// on_tile(EmTile) per tile.  A tile's input — for KT > 0 its A-operand rows (FAST: s in 11..16, one unguarded 16-byte
// load per lane; elements past the s classes are the row's own nucleotide floats, masked to 0), and the nucleotide
// floats of position n — is loaded two tiles ahead and classified one iteration later, so two tiles of loads are in
// flight per wave.
template <int KT, bool FAST, class Run, class Tile>
__device__ __forceinline__ void em_walk(const float *__restrict__ x, long long npos, int L, int s, int run_len, int tid,
                                        Run on_run, Tile on_tile) {
    const int w = s + 5, lane = tid & 63, g = lane >> 4, n = lane & 15;
    struct Raw { f4 xa[KT > 0 ? KT : 1]; EmNuc nu; };
    const long long nruns = (npos + run_len - 1) / run_len;
    const long long wave0 = (long long)blockIdx.x * (EM_THREADS / 64) + (tid >> 6);
    const long long nwaves = (long long)gridDim.x * (EM_THREADS / 64);
    for (long long run = wave0; run < nruns; run += nwaves) {
        const long long P0 = run * run_len;
        const long long left = npos - P0;
        const int ntiles = (int)((left < run_len ? left : run_len) + 15) / 16;
        // rows are addressed relative to the run with 32-bit offsets, clamped into the tensor
        const float *xrun = x + P0 * w;
        const int omin = (int)(-(P0 < 16 ? P0 : 16) * w);
        const int omax = (int)((left - 1 < run_len + 48 ? left - 1 : run_len + 48) * w);

        auto load_tile = [&](int rel) {                     // rel = tile's first row relative to P0
            Raw rw;
            int off = (rel + n) * w;
            off = off < omin ? omin : (off > omax ? omax : off);
            const float *xr = xrun + off;
#pragma unroll
            for (int kt = 0; kt < KT; ++kt) {
                f4 v;
                if (FAST) {
                    v = *reinterpret_cast<const f4u *>(xr + 4 * g);
                } else {
#pragma unroll
                    for (int kk = 0; kk < 4; ++kk) {
                        const int cls = 16 * kt + 4 * g + kk;
                        v[kk] = cls < s ? xr[cls] : 0.f;
                    }
                }
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) rw.xa[kt][kk] = (16 * kt + 4 * g + kk < s) ? v[kk] : 0.f;
            }
            rw.nu = em_load_nuc(xr, s);
            return rw;
        };

        EmTile<KT> t;
        t.tb = (int)(P0 % L);
        {
            const Raw rp = load_tile(-16);                  // codes only (clamped at the tensor start)
            const Raw r0 = load_tile(0);
            t.prev = em_classify(rp.nu, n);
            t.cur = em_classify(r0.nu, n);
#pragma unroll
            for (int kt = 0; kt < KT; ++kt) t.xa[kt] = r0.xa[kt];
        }
        Raw ra = load_tile(16);
        on_run(P0);
        for (int i = 0; i < ntiles; ++i) {
            t.P = P0 + 16 * i;
            const Raw rb = load_tile(16 * i + 32);          // two tiles ahead
            t.nxt = em_classify(ra.nu, n);
            on_tile(t);
            t.prev = t.cur; t.cur = t.nxt;
#pragma unroll
            for (int kt = 0; kt < KT; ++kt) t.xa[kt] = ra.xa[kt];
            ra = rb;
            t.tb += 16;
            if (t.tb >= L) t.tb %= L;
        }
    }
}

// A tile that is contiguous in memory leaves its stage flat: npieces 16-byte pieces, one per lane and round, of which
// nfl floats exist; the ragged end float by float.  accumulate (wave-uniform): add to what dst holds.  Piece -> lane is
// fixed, so a lane reads back what it stored itself.  NTS: nontemporal stores.
template <bool NTS>
__device__ __forceinline__ void em_flush_flat(const float *stage, float *dst, long long nfl, int npieces, int lane,
                                              bool accumulate) {
    for (int pc = lane; pc < npieces; pc += 64) {
        if (4 * pc + 3 < nfl) {
            f4 v = *reinterpret_cast<const f4 *>(stage + 4 * pc);
            if (accumulate) v += *reinterpret_cast<const f4 *>(dst + 4 * pc);
            if (NTS) __builtin_nontemporal_store(v, reinterpret_cast<f4 *>(dst + 4 * pc));
            else *reinterpret_cast<f4 *>(dst + 4 * pc) = v;
        } else {
            for (int u2 = 4 * pc; u2 < nfl; ++u2) dst[u2] = accumulate ? dst[u2] + stage[u2] : stage[u2];
        }
    }
}

#ifndef HMM_EM_NT
#define HMM_EM_NT 0         // 1: E leaves in nontemporal stores
#endif

// NT / KT: 16-state / 16-class tiles.  FAST: see em_walk.
template <int NT, int KT, bool FAST>
__global__ __launch_bounds__(EM_THREADS) void k_gene_emissions(const float *__restrict__ x, long long npos, int L, int s,
                                                               const float *__restrict__ B, int rows,
                                                               const int *__restrict__ state_row,
                                                               const float *__restrict__ codon, int nc,
                                                               const int *__restrict__ state_codon, int q,
                                                               float free_value, float add, float n_mass,
                                                               float *__restrict__ E) {
    extern __shared__ __attribute__((aligned(16))) float T9[];     // [2][max(nc,1)][512], then the output stages
    const int tid = threadIdx.x;
    const int w = s + 5;
    const int ncp = nc > 0 ? nc : 1;
    em_build_tables(T9, codon, nc, n_mass, tid);
    __syncthreads();

    const int lane = tid & 63, g = lane >> 4, n = lane & 15;
    // B-operand registers: Bexp[state 16 nt + n][class 16 kt + 4g + kk], and this lane's table rows
    f4 bw[NT][KT];
    int cj[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int j = 16 * nt + n;
        cj[nt] = j < q ? em_codon(state_codon, j, nc) : -1;
        const int brow = j < q ? em_row(state_row, j, rows) : 0;
#pragma unroll
        for (int kt = 0; kt < KT; ++kt)
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                const int cls = 16 * kt + 4 * g + kk;
                bw[nt][kt][kk] = (j < q && cls < s) ? B[brow * s + cls] : 0.f;
            }
    }
    const f4 zero4 = {0.f, 0.f, 0.f, 0.f};
    // this wave's output stage: one tile = 16 rows x q floats, contiguous in E
    float *stage = T9 + (size_t)2 * ncp * 512 + (size_t)(tid >> 6) * (16 * q);
    const int npieces = 4 * q;                              // 16-byte pieces per tile

    em_walk<KT, FAST>(x, npos, L, s, EM_RUN, tid, [](long long) {}, [&](const EmTile<KT> &t) {
        f4 D[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            D[nt] = zero4;
#pragma unroll
            for (int kt = 0; kt < KT; ++kt) D[nt] = mfma4v(t.xa[kt], bw[nt][kt], D[nt]);
        }
        em_scale_tile<NT>(D, stage, q, cj, q, T9, ncp, t.prev, t.cur, t.nxt, t.tb, L, t.P, npos, g, n, x, s, w, free_value,
                          add, n_mass);
        __builtin_amdgcn_wave_barrier();                    // stage is wave-private: LDS ops of a wave execute in order
        // the tile is 64 q contiguous bytes of E
        em_flush_flat<HMM_EM_NT != 0>(stage, E + t.P * q, (npos - t.P < 16 ? npos - t.P : 16) * q, npieces, lane, false);
        __builtin_amdgcn_wave_barrier();
    });
}

// ---- up to 256 states and 256 emission-kernel rows: hmm_gene_emissions_wide.  Same arguments, same values:
// GenePredHMMEmitter.forward for the models of three and more copies (1 + 14 c states; 43, 57, 71 .. 253 for c = 3 .. 18).
//
// Shape of the kernel: k_gene_emissions<4, 2, false>'s body with a loop over groups of 64 states inside the tile.  A
// wave owns runs of `run_len` positions (emw_run_len: 1024, shorter where b L would otherwise leave CUs idle; the values
// do not depend on it), walks them 16 at a time, and per tile and group:
//   * loads the group's B-operand registers bw[4][2] and table rows cj[4] from LDS.  The expanded emission kernel
//     Bexp (q x 32 classes, zero-padded) no longer fits the registers, so the workgroup stages it once (row stride 36
//     floats: the 16 lanes of a row group read 16-byte pieces 144 bytes apart, which spreads them over the banks; at
//     stride 32 they would all start in the same bank);
//   * issues the same v_mfma_f32_16x16x4_f32 chain over the classes as k_gene_emissions<4, 2> (same order, same
//     bits) and em_scale_tile with the group's slice of state_codon;
//   * flushes the 16 positions x 64 states rectangle from the wave's stage (row stride 68 floats): a row's piece is
//     256 contiguous bytes of E, written as 16-byte stores, 16 lanes per row.  E's rows are q floats long and q is
//     odd for every gene model, so these stores are 4-byte aligned only (global_store_dwordx4 takes that); the last
//     group is masked at q, its ragged end written float by float.
// Nothing depends on the grid: a position's values come from its own window and the staged tables.
//
// LDS per workgroup: tables 2 max(nc,1) x 2 KiB (36 KiB for the gene models' nc = 9) + Bexp 64 ngrp x 144 B +
// state_codon 64 ngrp x 4 B + 8 stages of 4352 B: 71 680 + 9472 ngrp bytes, 109 568 B at 256 states.  One
// workgroup per CU (160 KiB), i.e. two waves per SIMD.

#define EMW_MAXQ 256        // states
#define EMW_MAXR 256        // emission-kernel rows
#define EMW_BS 36           // row stride of Bexp in LDS (floats)
#define EMW_SS 68           // row stride of a wave's output stage (floats)

__global__ __launch_bounds__(EM_THREADS) void k_gene_emissions_wide(const float *__restrict__ x, long long npos, int L, int s,
                                                                    const float *__restrict__ B, int rows,
                                                                    const int *__restrict__ state_row,
                                                                    const float *__restrict__ codon, int nc,
                                                                    const int *__restrict__ state_codon, int q,
                                                                    float free_value, float add, float n_mass,
                                                                    int run_len, float *__restrict__ E) {
    constexpr int NT = 4, KT = 2;
    extern __shared__ __attribute__((aligned(16))) float T9[];     // [2][max(nc,1)][512], Bexp, state_codon, the stages
    const int tid = threadIdx.x;
    const int w = s + 5;
    const int ncp = nc > 0 ? nc : 1;
    const int ngrp = (q + 63) >> 6, qp = 64 * ngrp;
    float *Bx = T9 + (size_t)2 * ncp * 512;                        // [qp][EMW_BS]
    int *cjs = reinterpret_cast<int *>(Bx + (size_t)qp * EMW_BS);  // [qp]
    float *stage = reinterpret_cast<float *>(cjs + qp) + (size_t)(tid >> 6) * (16 * EMW_SS);
    em_build_tables(T9, codon, nc, n_mass, tid);
    for (int e = tid; e < qp * 32; e += EM_THREADS) {
        const int j = e >> 5, cls = e & 31;
        Bx[j * EMW_BS + cls] = (j < q && cls < s) ? B[(size_t)em_row(state_row, j, rows) * s + cls] : 0.f;
    }
    for (int j = tid; j < qp; j += EM_THREADS) cjs[j] = j < q ? em_codon(state_codon, j, nc) : -1;
    __syncthreads();

    const int lane = tid & 63, g = lane >> 4, n = lane & 15;
    const f4 zero4 = {0.f, 0.f, 0.f, 0.f};

    em_walk<KT, false>(x, npos, L, s, run_len, tid, [](long long) {}, [&](const EmTile<KT> &t) {
        const int nrow = (int)(npos - t.P < 16 ? npos - t.P : 16);          // rows of the tile that exist
#pragma unroll 1
        for (int grp = 0; grp < ngrp; ++grp) {
            const int j0 = 64 * grp;
            f4 D[NT];
            int cj[NT];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const int j = j0 + 16 * nt + n;
                cj[nt] = cjs[j];
                D[nt] = zero4;
#pragma unroll
                for (int kt = 0; kt < KT; ++kt) {
                    const f4 bw = *reinterpret_cast<const f4 *>(Bx + j * EMW_BS + 16 * kt + 4 * g);
                    D[nt] = mfma4v(t.xa[kt], bw, D[nt]);
                }
            }
            em_scale_tile<NT>(D, stage, EMW_SS, cj, q - j0, T9, ncp, t.prev, t.cur, t.nxt, t.tb, L, t.P, npos, g, n, x, s, w,
                              free_value, add, n_mass);
            __builtin_amdgcn_wave_barrier();                // stage is wave-private: LDS ops of a wave execute in order
            {   // flush: 16 lanes per row, 16 bytes each; rows 4 it + g
                const int c0 = j0 + 4 * n;                  // first state of this lane's piece
#pragma unroll
                for (int it = 0; it < 4; ++it) {
                    const int pl = 4 * it + g;
                    if (pl < nrow) {
                        const float *src = stage + pl * EMW_SS + 4 * n;
                        float *dst = E + (t.P + pl) * q + c0;
                        if (c0 + 3 < q) {
                            *reinterpret_cast<f4u *>(dst) = *reinterpret_cast<const f4 *>(src);
                        } else {
                            for (int u2 = 0; c0 + u2 < q; ++u2) dst[u2] = src[u2];
                        }
                    }
                }
            }
            __builtin_amdgcn_wave_barrier();
        }
    });
}

// ---- host side of the four gene entry points (hmm_emitter_grad.inc holds the two backward ones)

// shape, limits (maxq states, maxr rows), the pointers every entry point takes; others_ok: the entry point's own
static int em_check_args(int b, int L, int s, int q, int rows, int nc, int maxq, int maxr, const void *x, const void *B,
                         const void *state_row, const void *codon, const void *state_codon, bool others_ok) {
    if (b < 1 || L < 1 || s < 1 || q < 1 || rows < 1 || nc < 0) return HMM_ERR_BAD_SHAPE;
    if (q > maxq || s > EM_MAXS || rows > maxr || nc > EM_MAXC) return HMM_ERR_Q_UNSUPPORTED;
    if (!x || !B || !state_row || !state_codon || (nc > 0 && !codon) || !others_ok) return HMM_ERR_NULL_POINTER;
    return HMM_OK;
}

// positions per wave run of the wide kernels: EM_RUN, or less where that would leave fewer than 256 workgroups of 8
// runs (one workgroup per CU): b L / 2048 rounded up to whole tiles, at least 64.  A function of b L alone.
static int emw_run_len(long long npos) {
    long long r = (npos + 2047) / 2048;
    r = (r + 15) & ~15ll;
    return (int)(r < 64 ? 64 : (r > EM_RUN ? EM_RUN : r));
}

// workgroups that give every wave one run
static long long em_blocks(long long npos, int run_len) {
    const int wpb = EM_THREADS / 64;
    return ((npos + run_len - 1) / run_len + wpb - 1) / wpb;
}

// dynamic LDS of the forwards: the tables, then 8 stages of 16 x q floats, or (wide) Bexp, state_codon and 8 stages of
// 16 x EMW_SS
static size_t em_lds_bytes(int nc, int q, bool wide) {
    const size_t qp = (size_t)((q + 63) / 64) * 64, nst = EM_THREADS / 64;
    return ((size_t)2 * (nc > 0 ? nc : 1) * 512 + (wide ? qp * EMW_BS + qp + nst * 16 * EMW_SS : nst * 16 * q)) * sizeof(float);
}

extern "C" int hmm_gene_emissions(const float *x, int b, int L, int s, const float *B, int rows,
                                  const int *state_row, const float *codon, int nc, const int *state_codon, int q,
                                  float free_value, float add, int n_mass, float *E, void *stream) {
    if (int err = em_check_args(b, L, s, q, rows, nc, EM_MAXQ, EM_MAXR, x, B, state_row, codon, state_codon, E != nullptr))
        return err;
    const long long npos = (long long)b * L;
    const size_t lds = em_lds_bytes(nc, q, false);
    const long long nblk = em_blocks(npos, EM_RUN);
    const dim3 grid((unsigned)(nblk < 256 * 4 ? nblk : 256 * 4));
    hipStream_t st = (hipStream_t)stream;
#define EM_LAUNCH(NT_, KT_, FAST_)                                                                                       \
    hipLaunchKernelGGL((k_gene_emissions<NT_, KT_, FAST_>), grid, dim3(EM_THREADS), lds, st, x, npos, L, s, B, rows,      \
                       state_row, codon, nc, state_codon, q, free_value, add, (float)n_mass, E)
    if (q <= 16 && s >= 11 && s <= 16) EM_LAUNCH(1, 1, true);
    else if (q <= 16 && s <= 16) EM_LAUNCH(1, 1, false);
    else EM_LAUNCH(4, 2, false);
#undef EM_LAUNCH
    return check_launch();
}

extern "C" int hmm_gene_emissions_wide_max_states(void) { return EMW_MAXQ; }

extern "C" int hmm_gene_emissions_wide(const float *x, int b, int L, int s, const float *B, int rows,
                                       const int *state_row, const float *codon, int nc, const int *state_codon, int q,
                                       float free_value, float add, int n_mass, float *E, void *stream) {
    if (int err = em_check_args(b, L, s, q, rows, nc, EMW_MAXQ, EMW_MAXR, x, B, state_row, codon, state_codon, E != nullptr))
        return err;
    const long long npos = (long long)b * L;
    const int run_len = emw_run_len(npos);
    const long long nblk = em_blocks(npos, run_len);
    const dim3 grid((unsigned)(nblk < 256 * 4 ? nblk : 256 * 4));
    hipLaunchKernelGGL(k_gene_emissions_wide, grid, dim3(EM_THREADS), em_lds_bytes(nc, q, true), (hipStream_t)stream, x, npos,
                       L, s, B, rows, state_row, codon, nc, state_codon, q, free_value, add, (float)n_mass, run_len, E);
    return check_launch();
}
