// hmm_emitter_wide.inc — the fused gene emitter (hmm_emitter.inc) for up to 256 states and 256 emission-kernel
// rows, included by hmm_engine.hip after hmm_emitter.inc.  Same arguments, same values: GenePredHMMEmitter.forward
// for the models of three and more copies (1 + 14 c states; 43, 57, 71 .. 253 for c = 3 .. 18).
//
// Shape of the kernel: hmm_emitter.inc's <NT = 4, KT = 2> body with a loop over groups of 64 states inside the
// tile.  A wave owns runs of `run` positions (emw_run_len: 1024, shorter where b L would otherwise leave CUs idle;
// the values do not depend on it), walks them 16 at a time, classifies the tile's window once, and then,
// per group:
//   * loads the group's B-operand registers bw[4][2] and table rows cj[4] from LDS.  The expanded emission kernel
//     Bexp (q x 32 classes, zero-padded, state_row clamped into 0..rows-1) no longer fits the registers, so the
//     workgroup stages it once (row stride 36 floats: the 16 lanes of a row group read 16-byte pieces 144 bytes
//     apart, which spreads them over the banks; at stride 32 they would all start in the same bank);
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
// Compiler figures (gfx950, hipcc -O3): 196 VGPRs, no scratch, LDS as above (dynamic).

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
        float v = 0.f;
        if (j < q && cls < s) {
            int r = state_row[j];
            r = r < 0 ? 0 : (r >= rows ? rows - 1 : r);
            v = B[(size_t)r * s + cls];
        }
        Bx[j * EMW_BS + cls] = v;
    }
    for (int j = tid; j < qp; j += EM_THREADS) {
        int c = j < q ? state_codon[j] : -1;
        cjs[j] = c < nc ? c : nc - 1;                              // (nc = 0: every state is free)
    }
    __syncthreads();

    const int lane = tid & 63, g = lane >> 4, n = lane & 15;
    const f4 zero4 = {0.f, 0.f, 0.f, 0.f};

    struct Raw { f4 xa[KT]; EmNuc nu; };

    const long long nruns = (npos + run_len - 1) / run_len;
    const long long wave0 = (long long)blockIdx.x * (EM_THREADS / 64) + (tid >> 6);
    const long long nwaves = (long long)gridDim.x * (EM_THREADS / 64);
    for (long long run = wave0; run < nruns; run += nwaves) {
        const long long P0 = run * run_len;
        const long long left = npos - P0;
        const int ntiles = (int)((left < run_len ? left : run_len) + 15) / 16;
        int tb = (int)(P0 % L);                             // position of the tile's first row in its sequence
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
            for (int kt = 0; kt < KT; ++kt)
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) {
                    const int cls = 16 * kt + 4 * g + kk;
                    rw.xa[kt][kk] = cls < s ? xr[cls] : 0.f;
                }
            rw.nu = em_load_nuc(xr, s);
            return rw;
        };

        EmCodes prev, cur;
        f4 xa[KT];
        {
            const Raw rp = load_tile(-16);                  // codes only (clamped at the tensor start)
            const Raw r0 = load_tile(0);
            prev = em_classify(rp.nu, n);
            cur = em_classify(r0.nu, n);
#pragma unroll
            for (int kt = 0; kt < KT; ++kt) xa[kt] = r0.xa[kt];
        }
        Raw ra = load_tile(16);
        for (int i = 0; i < ntiles; ++i) {
            const int rel = 16 * i;
            const long long P = P0 + rel;
            const Raw rb = load_tile(rel + 32);             // two tiles ahead
            const EmCodes nxt = em_classify(ra.nu, n);
            const int nrow = (int)(npos - P < 16 ? npos - P : 16);          // rows of the tile that exist
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
                        D[nt] = mfma4v(xa[kt], bw, D[nt]);
                    }
                }
                em_scale_tile<NT>(D, stage, EMW_SS, cj, q - j0, T9, ncp, prev, cur, nxt, tb, L, P, npos, g, n, x, s, w,
                                  free_value, add, n_mass);
                __builtin_amdgcn_wave_barrier();            // stage is wave-private: LDS ops of a wave execute in order
                {   // flush: 16 lanes per row, 16 bytes each; rows 4 it + g
                    const int c0 = j0 + 4 * n;              // first state of this lane's piece
#pragma unroll
                    for (int it = 0; it < 4; ++it) {
                        const int pl = 4 * it + g;
                        if (pl < nrow) {
                            const float *src = stage + pl * EMW_SS + 4 * n;
                            float *dst = E + (P + pl) * q + c0;
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
            prev = cur; cur = nxt;
#pragma unroll
            for (int kt = 0; kt < KT; ++kt) xa[kt] = ra.xa[kt];
            ra = rb;
            tb += 16;
            if (tb >= L) tb %= L;
        }
    }
}

extern "C" int hmm_gene_emissions_wide_max_states(void) { return EMW_MAXQ; }

// positions per wave run: EM_RUN, or less where that would leave fewer than 256 workgroups of 8 runs (one workgroup
// per CU): b L / 2048 rounded up to whole tiles, at least 64.  A function of b L alone.
static int emw_run_len(long long npos) {
    long long r = (npos + 2047) / 2048;
    r = (r + 15) & ~15ll;
    return (int)(r < 64 ? 64 : (r > EM_RUN ? EM_RUN : r));
}

static size_t emw_lds_bytes(int nc, int q) {
    const size_t qp = (size_t)((q + 63) / 64) * 64;
    return ((size_t)2 * (nc > 0 ? nc : 1) * 512 + qp * EMW_BS + qp + (size_t)(EM_THREADS / 64) * 16 * EMW_SS) * sizeof(float);
}

extern "C" int hmm_gene_emissions_wide(const float *x, int b, int L, int s, const float *B, int rows,
                                       const int *state_row, const float *codon, int nc, const int *state_codon, int q,
                                       float free_value, float add, int n_mass, float *E, void *stream) {
    if (b < 1 || L < 1 || s < 1 || q < 1 || rows < 1 || nc < 0) return HMM_ERR_BAD_SHAPE;
    if (q > EMW_MAXQ || s > EM_MAXS || rows > EMW_MAXR || nc > EM_MAXC) return HMM_ERR_Q_UNSUPPORTED;
    if (!x || !B || !state_row || !state_codon || !E || (nc > 0 && !codon)) return HMM_ERR_NULL_POINTER;
    const long long npos = (long long)b * L;
    const int wpb = EM_THREADS / 64;
    const int run_len = emw_run_len(npos);
    const long long nblk = ((npos + run_len - 1) / run_len + wpb - 1) / wpb;
    const dim3 grid((unsigned)(nblk < 256 * 4 ? nblk : 256 * 4));
    hipLaunchKernelGGL(k_gene_emissions_wide, grid, dim3(EM_THREADS), emw_lds_bytes(nc, q), (hipStream_t)stream, x, npos, L, s,
                       B, rows, state_row, codon, nc, state_codon, q, free_value, add, (float)n_mass, run_len, E);
    return check_launch();
}
