// Epilogues of the SPLIT (fp32-grade) GEMM (gemm256_f16.hip): the 32 x 64 form of the launch-per-tile kernel and the 32 x 32 form of
// the persistent streaming kernel, both on ONE function that finishes and stores a lane's piece of a row: the same bits from both.
#pragma once
#include "gemm256_epilogue.h"

namespace ance {

// Output stores of the split epilogues are NON-TEMPORAL: the outputs of a launch (0.6-1.6 GB) are consumed by the next kernel and
// only pass through the 4 MB L2s on their way out, where they evict the operand panels the main loops re-read.  Same-box A/B
// (profiles/r05_ab_nt_store.jsonl, three alternations): FFN1 -0.7 %, the attention that follows the QKV GEMM -2.5 %, step +0.3 %.
// The pair-row epilogues move 8 columns per lane (16-byte hi and 16-byte lo accesses): an epilogue is bound by the NUMBER of
// vector-memory instructions its eight waves push through the CU's one address unit (~16 cycles each whatever their width) -- the
// fp32 store epilogue of QKV (32 dwordx4 stores per wave and tile) measured 4 us, the GELU pair epilogue with 8-byte accesses (64
// stores) 8.4 us, RESLN (64 loads + 64 stores + 32 statistics stores) 13.5 us.  Round 6: half as many, twice as wide.
__device__ __forceinline__ f16x8 cat_f16x4(const f16x4 a, const f16x4 b) { return f16x8{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]}; }
// columns n .. n + 7 (n a multiple of 8: inside one 32-column block)
__device__ __forceinline__ void epi_pair_store8_nt(const f32x4 va, const f32x4 vb, _Float16 *row, int W, int n) {
    f16x4 ha, ra, hb, rb;
    pair_split4(va, &ha, &ra);
    pair_split4(vb, &hb, &rb);
    __builtin_nontemporal_store(cat_f16x4(ha, hb), reinterpret_cast<f16x8 *>(row + pair_hi_col(n, W)));
    __builtin_nontemporal_store(cat_f16x4(ra, rb), reinterpret_cast<f16x8 *>(row + pair_lo_col(n, W)));
}

// slice statistics of the pair epilogues: a lane holds 8 columns of a row, 4 lanes a 32-column block, 8 lanes the 64-column slice
__device__ __forceinline__ float quad_sum(float x) {  // every lane of the quad ends with the same bits
    x += __builtin_amdgcn_update_dpp(0.f, x, 0xB1, 0xF, 0xF, true);   // quad_perm [1,0,3,2]
    x += __builtin_amdgcn_update_dpp(0.f, x, 0x4E, 0xF, 0xF, true);   // quad_perm [2,3,0,1]
    return x;
}
__device__ __forceinline__ float half_mirror(float x) { return __builtin_amdgcn_update_dpp(0.f, x, 0x141, 0xF, 0xF, true); }  // lane j <- lane 7 - j
__device__ __forceinline__ float sum8(const f32x4 a, const f32x4 b) { return ((a[0] + a[1]) + (a[2] + a[3])) + ((b[0] + b[1]) + (b[2] + b[3])); }
__device__ __forceinline__ float sumsq8(const f32x4 a, const f32x4 b, float m) {
    const float a0 = a[0] - m, a1 = a[1] - m, a2 = a[2] - m, a3 = a[3] - m, b0 = b[0] - m, b1 = b[1] - m, b2 = b[2] - m, b3 = b[3] - m;
    return ((a0 * a0 + a1 * a1) + (a2 * a2 + a3 * a3)) + ((b0 * b0 + b1 * b1) + (b2 * b2 + b3 * b3));
}

// Lane geometry of a read-back pass of PASS_COLS (64 or 32) columns.  Columns per lane: 8 for the pair-row outputs (16-byte hi and
// 16-byte lo accesses: 4 lanes write the 64 + 64 bytes of a pair block), 4 for the fp32 rows of QKV (with 8 columns a lane's two
// 16-byte stores would interleave with its neighbours' -- measured +3.5 % on that GEMM).
template <int EPI, int PASS_COLS>
struct SplitLanes {
    static constexpr int CPL = EPI == EPI_S_QKV ? 4 : 8, NV = CPL / 4;            // columns per lane, f32x4 per lane and row
    static constexpr int LPR = PASS_COLS / CPL, RPI = 64 / LPR, ITS = 32 / RPI;  // lanes per row, rows per instruction, instructions per pass
};

// A lane's piece of output row `row` (columns n .. n + CPL - 1; sp: where it lies in the wave's slab) finished and stored:
//   EPI_S_QKV / EPI_S_GELU   a <- r (acc winv - mu c) + b'  as  fma(acc, r winv, fma(-mu r, c, b'))  (winv is a power of two), GELU;
//   EPI_S_RESLN              a comes in finished (the residual arithmetic is the caller's) and sp is not read;
// then the range guard and the non-temporal store of the fp32 piece (QKV) or of the hi and lo pieces of the pair row.
// b / c: the piece's columns of b' and csum.  (contraction off: gemm256_gelu.h explains why a last bit otherwise depends on the
// register slot.)
template <int EPI>
__device__ __forceinline__ void split_piece_store(const GemmArgs &G, const float *sp, f32x4 (&a)[SplitLanes<EPI, 64>::NV],
                                                  const f32x4 (&b)[SplitLanes<EPI, 64>::NV], const f32x4 (&c)[SplitLanes<EPI, 64>::NV],
                                                  float mean, float rstd, float winv, size_t row, int n, float *vmax) {
#pragma clang fp contract(off)
    constexpr int NV = SplitLanes<EPI, 64>::NV;
    if constexpr (EPI != EPI_S_RESLN) {
#pragma unroll
        for (int h = 0; h < NV; ++h) a[h] = *reinterpret_cast<const f32x4 *>(sp + 4 * h);
    }
    const float mr = mean * rstd, rw = rstd * winv;  // r (acc winv) = acc (r winv)
#pragma unroll
    for (int h = 0; h < NV; ++h) {
        if constexpr (EPI != EPI_S_RESLN) {
#pragma unroll
            for (int e = 0; e < 4; ++e) a[h][e] = __builtin_fmaf(a[h][e], rw, __builtin_fmaf(-mr, c[h][e], b[h][e]));
            if constexpr (EPI == EPI_S_GELU) a[h] = gelu_exact4(a[h]);
        }
        range_track4(a[h], vmax);  // (QKV: the attention splits K and V into pairs while it stages them)
    }
    if constexpr (EPI == EPI_S_QKV) __builtin_nontemporal_store(a[0], reinterpret_cast<f32x4 *>(G.out32 + row * G.ldc + n));
    else epi_pair_store8_nt(a[0], a[NV - 1], G.out16 + row * G.ldc, G.N, n);
}

// One structure for the three of them: 4 passes over the wave's 128 rows, each through the wave-private fp32 slab
// [32 m][64 n] (as EPI_RES32 / EPI_RESLN), so that on read-back a lane owns 4 consecutive columns of a row and global
// traffic is whole 16-byte (fp32) or 8-byte (fp16) row segments.
//   EPI_S_QKV    out32[m][n]         = r (acc' - mu c) + b'                   folded LayerNorm, fp32 out (Q | K | V)
//   EPI_S_GELU   out16 pair [m][n]   = pair(gelu_exact(r (acc' - mu c) + b'))   pair row of 2 N halves (common.h), ldc = 2 N
//   EPI_S_RESLN  out16 pair [m][n]   = pair(acc' + bias + LayerNorm(residual pair)), + slice statistics (part_out)
// acc' = acc winv: winv is the inverse of the power of two the weight was stored with (exact; it rides on the row's rstd or in
// the one fma that adds the residual, so it costs no instruction).
// On read-back 16 lanes write 256 contiguous bytes of an fp32 row, 8 lanes the two pair blocks of a pair row (SplitLanes).
template <int EPI, int HW = 768>
__device__ __forceinline__ void gemm256_epilogue_split(const GemmArgs &G, f32x4 (&acc)[4][8], float *smem_f, int m0, int n0,
                                                       int w, int l, float winv) {
#pragma clang fp contract(off)
    const int i = l & 15, c4 = 4 * (l >> 4);  // acc[x][y] (16 x 16 blocks): n = nw0 + 16 x + c4 + (0..3), m = mw0 + 16 y + i
    const int wm = w >> 2, wn = w & 3;
    const int mw0 = m0 + wm * 128, nw0 = n0 + wn * 64;
    float *slab = smem_f + w * 4096;
    constexpr int LS = 68;
    typedef SplitLanes<EPI, 64> LN;
    constexpr int CPL = LN::CPL, NV = LN::NV, LPR = LN::LPR, RPI = LN::RPI, ITS = LN::ITS;
    const int cl = l % LPR, rl_ = l / LPR;
    const int nc = nw0 + cl * CPL;      // first of this lane's columns
    const float *pb = smem_f + EPB_OFF;
    const float *vp = pb + EPB_VEC + wn * 64 + cl * CPL;
    f32x4 v0[NV], v1[NV], v2[NV];       // bias (b' for the folded ones) | csum or gamma | beta
#pragma unroll
    for (int h = 0; h < NV; ++h) {
        v0[h] = *reinterpret_cast<const f32x4 *>(vp + 4 * h);
        v1[h] = *reinterpret_cast<const f32x4 *>(vp + 256 + 4 * h);
        v2[h] = f32x4{0.f, 0.f, 0.f, 0.f};
        if constexpr (EPI == EPI_S_RESLN) v2[h] = *reinterpret_cast<const f32x4 *>(vp + 512 + 4 * h);
    }
    const int n_parts = G.N >> 6, slice = nw0 >> 6;
    float vmax = 0.f;  // range guard: running maximum of |what this thread stores| (common.h)
#pragma unroll
    for (int y = 0; y < 4; ++y) {
        f16x8 rh[ITS], rl[ITS];
        float mean[ITS], rstd[ITS];
#pragma unroll
        for (int it = 0; it < ITS; ++it) {
            const int rr = it * RPI + rl_;
            if constexpr (EPI == EPI_S_RESLN) {
                const _Float16 *rp = G.res_hi + (size_t)(mw0 + y * 32 + rr) * G.ldr;
                rh[it] = *reinterpret_cast<const f16x8 *>(rp + pair_hi_col(nc, G.N));
                rl[it] = *reinterpret_cast<const f16x8 *>(rp + pair_lo_col(nc, G.N));
            }
            mean[it] = pb[EPB_STATS + 2 * (wm * 128 + y * 32 + rr)];
            rstd[it] = pb[EPB_STATS + 2 * (wm * 128 + y * 32 + rr) + 1];
        }
        epi_sync();
#pragma unroll
        for (int yb = 0; yb < 2; ++yb)
#pragma unroll
            for (int x = 0; x < 4; ++x) *reinterpret_cast<f32x4 *>(slab + (yb * 16 + i) * LS + x * 16 + c4) = acc[x][2 * y + yb];
        epi_sync();
        f32x4 vv[ITS][NV];
#pragma unroll
        for (int it = 0; it < ITS; ++it) {
            const int rr = it * RPI + rl_;
            const size_t row = (size_t)(mw0 + y * 32 + rr);
            const float *sp = slab + rr * LS + cl * CPL;
            if constexpr (EPI == EPI_S_RESLN) {
#pragma unroll
                for (int h = 0; h < NV; ++h) {
                    f32x4 a = *reinterpret_cast<const f32x4 *>(sp + 4 * h);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float ga = rstd[it] * v1[h][e];
                        const float ra = (float)rh[it][4 * h + e] + (float)rl[it][4 * h + e] * PAIR_LO_INV;  // exact in fp32: 22 bits
                        a[e] = __builtin_fmaf(a[e], winv, __builtin_fmaf(ra - mean[it], ga, v0[h][e] + v2[h][e]));
                    }
                    vv[it][h] = a;
                }
            }
            split_piece_store<EPI>(G, sp, vv[it], v0, v1, mean[it], rstd[it], winv, row, nc, &vmax);
        }
        if constexpr (EPI == EPI_S_RESLN) {
            // (mean, M2) of the 64 columns of every row: lane sums of 8 columns, quad sums (32 columns), the two quads of the row
            float s4[ITS], q4[ITS];
#pragma unroll
            for (int it = 0; it < ITS; ++it) {
                const float s = quad_sum(sum8(vv[it][0], vv[it][NV - 1]));
                s4[it] = (s + half_mirror(s)) * (1.0f / 64.0f);
            }
#pragma unroll
            for (int it = 0; it < ITS; ++it) {
                const float q = quad_sum(sumsq8(vv[it][0], vv[it][NV - 1], s4[it]));
                q4[it] = q + half_mirror(q);
            }
            // every lane of a row holds the row's (s, q) of all ITS row groups: lane cl < ITS stores group cl -- ONE store instruction
            // for the 32 rows of the pass instead of ITS (the epilogue is bound by its vector-memory instruction count)
            static_assert(ITS == 4 && LPR >= 4, "one lane per row group");
            const float ss = cl == 0 ? s4[0] : cl == 1 ? s4[1] : cl == 2 ? s4[2] : s4[3];
            const float qq = cl == 0 ? q4[0] : cl == 1 ? q4[1] : cl == 2 ? q4[2] : q4[3];
            if constexpr (HW == 1024) {
                if (cl < ITS) epb_park_part(smem_f, wm * 128 + y * 32 + cl * RPI + rl_, wn, ss, qq);
            } else if (cl < ITS) {
                *reinterpret_cast<float2 *>(G.part_out + ((size_t)(mw0 + y * 32 + cl * RPI + rl_) * n_parts + slice) * 2) = make_float2(ss, qq);
            }
        }
    }
    if constexpr (EPI == EPI_S_RESLN && HW == 1024) epb_merge_parts(G, smem_f, m0, n0, w * 64 + l);
    range_report(vmax, G.range_faults);
}

// ---- epilogues of the STREAMING (persistent) split GEMM: EPI_S_QKV and EPI_S_GELU -----------------------------------------
// The same arithmetic, bit for bit (split_piece_store; tests/test_gpu_gemm.py compares the two kernels with array_equal), in the LDS the persistent
// kernel has left while the next output tile's first K-tiles are in flight in the stage buffers: a wave-private slab of [32 m][32 n]
// fp32 (row stride 36 floats: the 16-byte writes of 16 lanes fall into 16 different bank quads; 4.5 KiB per wave instead of the
// 16 KiB slices of the stage buffers the launch-per-tile kernel's epilogue reuses), EIGHT passes (y, x) of 32 rows x 32 columns.
// A 32-column block is exactly one [hi (32) | lo (32)] block of a pair row (common.h): on read-back a row of the pass is
// 8 lanes x 16 bytes = 128 contiguous bytes of fp32 (EPI_S_QKV) or 4 lanes x (16 + 16) = the 64 + 64 bytes of one pair block.
// (EPI_S_RESLN in this form -- residual rows requested a pass ahead, slice statistics combined over the passes x = 0, 1 -- measured
// 1.6-3.4 us per tile slower than the 32 x 64 form: commit abaa8b9, DESIGN_REJECTED.md round 6.)
// (EPS_LS, EPS_SLAB_FLOATS and where a wave's slab lies: gemm256_tile.h)
template <int EPI>
__device__ __forceinline__ void gemm256_epilogue_split32(const GemmArgs &G, f32x4 (&acc)[4][8], float *slab, const float *stats,
                                                         const float *vec, int m0, int n0, int w, int l, float winv) {
    static_assert(EPI == EPI_S_QKV || EPI == EPI_S_GELU, "the RESLN GEMMs run the launch-per-tile kernel (DESIGN_REJECTED.md round 6)");
    const int i = l & 15, c4 = 4 * (l >> 4);  // as gemm256_epilogue_split
    const int wm = w >> 2, wn = w & 3;
    const int mw0 = m0 + wm * 128, nw0 = n0 + wn * 64;
    constexpr int LS = EPS_LS;
    typedef SplitLanes<EPI, 32> LN;
    constexpr int CPL = LN::CPL, NV = LN::NV, LPR = LN::LPR, RPI = LN::RPI, ITS = LN::ITS;
    const int cl = l % LPR, rl_ = l / LPR;
    float vmax = 0.f;  // range guard (common.h)
#pragma unroll
    for (int p = 0; p < 8; ++p) {
        const int y = p >> 1, x = p & 1;
        const float *vp = vec + wn * 64 + x * 32 + cl * CPL;
        f32x4 v0[NV], v1[NV];  // b' | csum
#pragma unroll
        for (int h = 0; h < NV; ++h) {
            v0[h] = *reinterpret_cast<const f32x4 *>(vp + 4 * h);
            v1[h] = *reinterpret_cast<const f32x4 *>(vp + 256 + 4 * h);
        }
        epi_sync();
#pragma unroll
        for (int yb = 0; yb < 2; ++yb)
#pragma unroll
            for (int xb = 0; xb < 2; ++xb) *reinterpret_cast<f32x4 *>(slab + (yb * 16 + i) * LS + xb * 16 + c4) = acc[2 * x + xb][2 * y + yb];
        epi_sync();
#pragma unroll
        for (int it = 0; it < ITS; ++it) {
            const int rr = it * RPI + rl_;
            const float mean = stats[2 * (wm * 128 + y * 32 + rr)], rstd = stats[2 * (wm * 128 + y * 32 + rr) + 1];
            f32x4 vv[NV];
            split_piece_store<EPI>(G, slab + rr * LS + cl * CPL, vv, v0, v1, mean, rstd, winv, (size_t)(mw0 + y * 32 + rr), nw0 + x * 32 + cl * CPL, &vmax);
        }
    }
    range_report(vmax, G.range_faults);
}

}  // namespace ance
