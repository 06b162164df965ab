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

// ---- pieces shared with the backward (hmm_emitter_grad.inc)

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

// NT / KT: 16-state / 16-class tiles.  FAST: s in 11..16, rows loaded with one unguarded 16-byte
// load per lane (elements past the s classes are the row's own nucleotide floats, masked to 0).
template <int NT, int KT, bool FAST>
#ifndef HMM_EM_NT
#define HMM_EM_NT 0
#endif
__global__ __launch_bounds__(EM_THREADS) void k_gene_emissions(const float *__restrict__ x, long long npos, int L, int s,
                                                               const float *__restrict__ B,
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
        cj[nt] = j < q ? state_codon[j] : -1;
        const int brow = j < q ? state_row[j] : 0;
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

    struct Raw { f4 xa[KT]; EmNuc nu; };

    const long long nruns = (npos + EM_RUN - 1) / EM_RUN;
    const long long wave0 = (long long)blockIdx.x * (EM_THREADS / 64) + (tid >> 6);
    const long long nwaves = (long long)gridDim.x * (EM_THREADS / 64);
    for (long long run = wave0; run < nruns; run += nwaves) {
        const long long P0 = run * EM_RUN;
        const long long left = npos - P0;
        const int ntiles = (int)((left < EM_RUN ? left : EM_RUN) + 15) / 16;
        int tb = (int)(P0 % L);                             // position of the tile's first row in its sequence
        // rows are addressed relative to the run with 32-bit offsets, clamped into the tensor
        const float *xrun = x + P0 * w;
        const int omin = (int)(-(P0 < 16 ? P0 : 16) * w);
        const int omax = (int)((left - 1 < EM_RUN + 48 ? left - 1 : EM_RUN + 48) * w);

        // one tile's input: A-operand rows and the nucleotide floats of position m (classified one
        // iteration later, so two tiles of loads are in flight per wave)
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
        auto classify = [&](const Raw &rw) { return em_classify(rw.nu, n); };

        EmCodes prev, cur;
        f4 xa[KT];
        {
            const Raw rp = load_tile(-16);                  // codes only (clamped at the tensor start)
            const Raw r0 = load_tile(0);
            prev = classify(rp);
            cur = classify(r0);
#pragma unroll
            for (int kt = 0; kt < KT; ++kt) xa[kt] = r0.xa[kt];
        }
        Raw ra = load_tile(16);
        for (int i = 0; i < ntiles; ++i) {
            const int rel = 16 * i;
            const long long P = P0 + rel;
            const Raw rb = load_tile(rel + 32);             // two tiles ahead
            f4 D[NT];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                D[nt] = zero4;
#pragma unroll
                for (int kt = 0; kt < KT; ++kt) D[nt] = mfma4v(xa[kt], bw[nt][kt], D[nt]);
            }
            const EmCodes nxt = classify(ra);
            em_scale_tile<NT>(D, stage, q, cj, q, T9, ncp, prev, cur, nxt, tb, L, P, npos, g, n, x, s, w, free_value, add,
                              n_mass);
            __builtin_amdgcn_wave_barrier();                // stage is wave-private: LDS ops of a wave execute in order
            {   // flush the tile: 64 q contiguous bytes of E, 16 bytes per lane
                const long long nfl = (npos - P < 16 ? npos - P : 16) * q;      // floats that exist
                float *dst = E + P * q;
                for (int pc = lane; pc < npieces; pc += 64) {
                    if (4 * pc + 3 < nfl) {
#if HMM_EM_NT
                        __builtin_nontemporal_store(*reinterpret_cast<const f4 *>(stage + 4 * pc), reinterpret_cast<f4 *>(dst + 4 * pc));
#else
                        *reinterpret_cast<f4 *>(dst + 4 * pc) = *reinterpret_cast<const f4 *>(stage + 4 * pc);
#endif
                    } else {
                        for (int u2 = 4 * pc; u2 < nfl; ++u2) dst[u2] = stage[u2];
                    }
                }
            }
            __builtin_amdgcn_wave_barrier();
            prev = cur; cur = nxt;
#pragma unroll
            for (int kt = 0; kt < KT; ++kt) xa[kt] = ra.xa[kt];
            ra = rb;
            tb += 16;
            if (tb >= L) tb %= L;
        }
    }
}

extern "C" int hmm_gene_emissions(const float *x, int b, int L, int s, const float *B, int rows,
                                  const int *state_row, const float *codon, int nc, const int *state_codon, int q,
                                  float free_value, float add, int n_mass, float *E, void *stream) {
    if (b < 1 || L < 1 || s < 1 || q < 1 || rows < 1 || nc < 0) return HMM_ERR_BAD_SHAPE;
    if (q > EM_MAXQ || s > EM_MAXS || rows > EM_MAXR || nc > EM_MAXC) return HMM_ERR_Q_UNSUPPORTED;
    if (!x || !B || !state_row || !state_codon || !E || (nc > 0 && !codon)) return HMM_ERR_NULL_POINTER;
    const long long npos = (long long)b * L;
    const size_t lds = ((size_t)2 * (nc > 0 ? nc : 1) * 512 + (size_t)(EM_THREADS / 64) * 16 * q) * sizeof(float);
    const int wpb = EM_THREADS / 64;
    const long long nblk = ((npos + EM_RUN - 1) / EM_RUN + wpb - 1) / wpb;
    const dim3 grid((unsigned)(nblk < 256 * 4 ? nblk : 256 * 4));
    hipStream_t st = (hipStream_t)stream;
#define EM_LAUNCH(NT_, KT_, FAST_)                                                                                       \
    hipLaunchKernelGGL((k_gene_emissions<NT_, KT_, FAST_>), grid, dim3(EM_THREADS), lds, st, x, npos, L, s, B, state_row, \
                       codon, nc, state_codon, q, free_value, add, (float)n_mass, E)
    if (q <= 16 && s >= 11 && s <= 16) EM_LAUNCH(1, 1, true);
    else if (q <= 16 && s <= 16) EM_LAUNCH(1, 1, false);
    else EM_LAUNCH(4, 2, false);
#undef EM_LAUNCH
    return check_launch();
}
