// Epilogues of the 256 x 256 fp16 GEMM kernel (gemm256_f16.hip: gemm256_f16_desc_kernel).
// Swapped MFMA orientation: acc[x][y][r] holds  n = n0 + wn*64 + x*32 + (r&3) + 8*(r>>2) + 4*g,
// m = m0 + wm*128 + y*32 + i  -- a lane owns one output row m and 4 consecutive n per register
// quad, staged through a wave-private 16 KiB LDS slab so that global traffic is whole 16-byte row
// segments.  Must be entered by all 512 threads after the last LDS read of the main loop.
// The split GEMM's epilogues are in gemm256_epilogue_split.h; the parameter block they all read is laid out in gemm256_tile.h.
#pragma once
#include "gemm256_gelu.h"
#include "gemm256_tile.h"

namespace ance {

// The slabs are wave-private and, once the main loop has returned, no wave reads the stage buffers any more
// (pipe256.h: the last barrier every wave passes comes after the last LDS read of both wave groups), so the write ->
// read-back -> next-pass-write ordering inside a slab is a matter of ONE wave: LDS operations of a wave execute in order,
// and a wavefront-scope fence keeps the compiler from moving a lane's read above another lane's write.  Workgroup barriers
// here cost two per pass that make all eight waves wait for the slowest one.
__device__ __forceinline__ void epi_sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// EPI_RES32 / EPI_RESLN: the 32 rows x 64 columns of pass y go through the wave-private slab [32 m][64 n] fp32, row stride 68
// floats, so that on read-back 16 lanes cover one row (lane l: columns 4 (l & 15) .. + 3), 4 rows per instruction
constexpr int RES_LS = 68;
__device__ __forceinline__ void res_slab_write(float *slab, const f32x16 (&acc)[2][4], int y, int l) {
    const int g = l >> 5, i = l & 31;
    epi_sync();
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int rq = 0; rq < 4; ++rq) {
            const f32x16 &a = acc[x][y];
            *reinterpret_cast<f32x4 *>(slab + i * RES_LS + x * 32 + 8 * rq + 4 * g) =
                f32x4{a[4 * rq], a[4 * rq + 1], a[4 * rq + 2], a[4 * rq + 3]};
        }
    epi_sync();
}
__device__ __forceinline__ f32x4 res_slab_read(const float *slab, int it, int l) {  // row it * 4 + (l >> 4) of the pass
    return *reinterpret_cast<const f32x4 *>(slab + (it * 4 + (l >> 4)) * RES_LS + (l & 15) * 4);
}

template <int EPI_, int HW = 768>
__device__ __forceinline__ void gemm256_epilogue(const GemmArgs &G, f32x16 (&acc)[2][4], float *smem_f, int m0, int n0,
                                                 int w, int l, unsigned long long *pass_stamps = nullptr) {
    _Float16 *smem = reinterpret_cast<_Float16 *>(smem_f);
    const int g = l >> 5, i = l & 31;
    const int wm = w >> 2, wn = w & 3;
    // acc[x][y][r]: n = n0 + wn*64 + x*32 + (r&3) + 8*(r>>2) + 4*g ;  m = m0 + wm*128 + y*32 + i
    const int mw0 = m0 + wm * 128, nw0 = n0 + wn * 64;
    constexpr bool FOLD = EPI_ == EPI_QK_F || EPI_ == EPI_GELU_F || EPI_ == EPI_VT_F;
    constexpr int EPI = EPI_ == EPI_QK_F ? EPI_QK : EPI_ == EPI_GELU_F ? EPI_GELU : EPI_ == EPI_VT_F ? EPI_VT : EPI_;
    if constexpr (EPI == EPI_VT) {  // (EPI_VT_F only)
        // Output rows are A-matrix rows m (features, bias per row); columns are tokens n scattered
        // through col_map (per-sequence 8-aligned key columns, so 16-byte stores are impossible in
        // general).  Slab [64 m][64 n] halves per pass; on read-back a lane owns ONE token column and
        // walks the 64 feature rows: every store instruction writes 64 consecutive tokens = 128 B of
        // one V^T row, and col_map is read once per lane.
        _Float16 *slab = smem + w * 8192;
        constexpr int LS = 72;
        const int ntok = nw0 + l;
        const bool tok_ok = ntok < G.n_valid;
        const int col = tok_ok ? G.col_map[ntok] : 0;
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            epi_sync();
            float bias[2], cs[2];  // per-lane row (feature) constants of the two 32-row blocks of this pass
#pragma unroll
            for (int yy = 0; yy < 2; ++yy) {
                bias[yy] = smem_f[EPB_OFF + EPB_VEC + wm * 128 + (2 * p + yy) * 32 + i];
                cs[yy] = smem_f[EPB_OFF + EPB_VEC + 256 + wm * 128 + (2 * p + yy) * 32 + i];
            }
#pragma unroll
            for (int x = 0; x < 2; ++x)
#pragma unroll
                for (int rq = 0; rq < 4; ++rq) {
                    // tokens are the columns -- (mean, rstd) of 4 consecutive tokens = 32 bytes of LDS, read once per pass and
                    // column quad; r (acc - mu c) + b = acc r + (b - (mu r) c)
                    const float *sp = smem_f + EPB_OFF + EPB_STATS + 2 * (wn * 64 + x * 32 + 8 * rq + 4 * g);
                    const f32x4 s01 = *reinterpret_cast<const f32x4 *>(sp);
                    const f32x4 s23 = *reinterpret_cast<const f32x4 *>(sp + 4);
                    const f32x4 r4 = f32x4{s01[1], s01[3], s23[1], s23[3]};
                    const f32x4 mr4 = f32x4{s01[0] * s01[1], s01[2] * s01[3], s23[0] * s23[1], s23[2] * s23[3]};
#pragma unroll
                    for (int yy = 0; yy < 2; ++yy) {
                        const f32x16 &a = acc[x][2 * p + yy];
                        f32x4 t = f32x4{a[4 * rq], a[4 * rq + 1], a[4 * rq + 2], a[4 * rq + 3]};
                        t = t * r4 + (bias[yy] - mr4 * cs[yy]);
                        *reinterpret_cast<f16x4 *>(slab + (yy * 32 + i) * LS + x * 32 + 8 * rq + 4 * g) =
                            f16x4{(_Float16)t[0], (_Float16)t[1], (_Float16)t[2], (_Float16)t[3]};
                    }
                }
            epi_sync();
            if (tok_ok) {
                _Float16 *obase = G.out16 + (size_t)(mw0 + p * 64) * G.ldc + col;
#pragma unroll 8
                for (int rr = 0; rr < 64; ++rr) obase[(size_t)rr * G.ldc] = slab[rr * LS + l];
            }
        }
    } else if constexpr (EPI == EPI_RES32) {
        // 4 passes over the wave's 128 rows, each through the wave's slab (res_slab_write / res_slab_read)
        float *slab = smem_f + w * 4096;  // 16 KiB per wave
        const int c4 = l & 15;
        const f32x4 bias = *reinterpret_cast<const f32x4 *>(G.bias + nw0 + c4 * 4);
#pragma unroll
        for (int y = 0; y < 4; ++y) {
            // residual rows of this pass: issued first so their latency hides behind the LDS round trip
            f32x4 res[8];
#pragma unroll
            for (int it = 0; it < 8; ++it) {
                const int rr = it * 4 + (l >> 4);
                res[it] = *reinterpret_cast<const f32x4 *>(G.res32 + (size_t)(mw0 + y * 32 + rr) * G.ldc + nw0 + c4 * 4);
            }
            res_slab_write(slab, acc, y, l);
            // read back: 8 instructions
#pragma unroll
            for (int it = 0; it < 8; ++it) {
                const int rr = it * 4 + (l >> 4);
                const f32x4 v = res_slab_read(slab, it, l);
                *reinterpret_cast<f32x4 *>(G.out32 + (size_t)(mw0 + y * 32 + rr) * G.ldc + nw0 + c4 * 4) = v + bias + res[it];
            }
        }
    } else if constexpr (EPI == EPI_RESLN) {
        // as EPI_RES32, with the residual stream as an fp16 pair: v = acc + bias + LayerNorm(res_hi + res_lo);
        // out16 = fp16(v) (the next GEMM's token operand AND the high half of the stream), out_lo = fp16(v - out16)
        // (v - fp16(v) is exact in fp32; the pair carries 22 bits).  Per row and 64-column slice the (mean, M2) of v go
        // to part_out[] -- the consumers combine the N / 64 slices of a row (Chan) into (mean, rstd) in their own epilogues.
        float *slab = smem_f + w * 4096;
        const int c4 = l & 15;
        const float *pb = smem_f + EPB_OFF;
        const f32x4 lng = *reinterpret_cast<const f32x4 *>(pb + EPB_VEC + 256 + wn * 64 + c4 * 4);
        const f32x4 bias_beta = *reinterpret_cast<const f32x4 *>(pb + EPB_VEC + wn * 64 + c4 * 4) +
                                *reinterpret_cast<const f32x4 *>(pb + EPB_VEC + 512 + wn * 64 + c4 * 4);
        const int n_parts = G.N >> 6, slice = nw0 >> 6;
#pragma unroll
        for (int y = 0; y < 4; ++y) {
            f16x4 rh[8], rl[8];
            float mean[8], rstd[8];
#pragma unroll
            for (int it = 0; it < 8; ++it) {
                const int rr = it * 4 + (l >> 4);
                const size_t row = (size_t)(mw0 + y * 32 + rr);
                rh[it] = *reinterpret_cast<const f16x4 *>(G.res_hi + row * G.ldc + nw0 + c4 * 4);
                rl[it] = *reinterpret_cast<const f16x4 *>(G.res_lo + row * G.ldc + nw0 + c4 * 4);
                mean[it] = pb[EPB_STATS + 2 * (wm * 128 + y * 32 + rr)];
                rstd[it] = pb[EPB_STATS + 2 * (wm * 128 + y * 32 + rr) + 1];
            }
            res_slab_write(slab, acc, y, l);
            // running pointers (a row step is 4 rows): 64-bit address arithmetic per store was a fifth of this loop
            const size_t row0 = (size_t)(mw0 + y * 32 + (l >> 4));
            _Float16 *ph = G.out16 + row0 * G.ldc + nw0 + c4 * 4;
            _Float16 *pl = G.out_lo + row0 * G.ldc + nw0 + c4 * 4;
            const size_t rstep = (size_t)4 * G.ldc;
            f32x4 vv[8];
#pragma unroll
            for (int it = 0; it < 8; ++it) {
                // acc + bias + LayerNorm(hi + lo) = acc + hi a + (lo a + (bias + beta - mean a)),  a = rstd gamma
                f32x4 v = res_slab_read(slab, it, l);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float a = rstd[it] * lng[e];
                    const float b0 = __builtin_fmaf(-mean[it], a, bias_beta[e]);
                    v[e] += __builtin_fmaf((float)rh[it][e], a, __builtin_fmaf((float)rl[it][e], a, b0));
                }
                const f16x4 hi = cvt_f16x4_pinned(v);
                const f16x4 lo = f16x4{(_Float16)(v[0] - (float)hi[0]), (_Float16)(v[1] - (float)hi[1]),
                                       (_Float16)(v[2] - (float)hi[2]), (_Float16)(v[3] - (float)hi[3])};
                *reinterpret_cast<f16x4 *>(ph + it * rstep) = hi;
                *reinterpret_cast<f16x4 *>(pl + it * rstep) = lo;
                vv[it] = v;
            }
            // slice statistics of the 8 rows together: eight independent 16-lane reductions, interleaved (gemm_f16.h: row16_sum8)
            float s8[8], q8[8];
#pragma unroll
            for (int it = 0; it < 8; ++it) s8[it] = (vv[it][0] + vv[it][1]) + (vv[it][2] + vv[it][3]);
            row16_sum8(s8);
#pragma unroll
            for (int it = 0; it < 8; ++it) {
                const float m64 = s8[it] * (1.0f / 64.0f);
                s8[it] = m64;
                const float d0 = vv[it][0] - m64, d1 = vv[it][1] - m64, d2 = vv[it][2] - m64, d3 = vv[it][3] - m64;
                q8[it] = (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
            }
            row16_sum8(q8);
            if constexpr (HW == 1024) {
                if (c4 == 0) {
#pragma unroll
                    for (int it = 0; it < 8; ++it) epb_park_part(smem_f, wm * 128 + y * 32 + it * 4 + (l >> 4), wn, s8[it], q8[it]);
                }
            } else if (c4 == 0) {
                float *pp = G.part_out + (row0 * n_parts + slice) * 2;
                const size_t pstep = (size_t)4 * n_parts * 2;
#pragma unroll
                for (int it = 0; it < 8; ++it) *reinterpret_cast<float2 *>(pp + it * pstep) = make_float2(s8[it], q8[it]);
            }
#ifdef ANCE_MEASURE
            if (pass_stamps && w == 0 && l == 0) pass_stamps[y] = __builtin_amdgcn_s_memrealtime();
#endif
        }
        if constexpr (HW == 1024) epb_merge_parts(G, smem_f, m0, n0, w * 64 + l);
    } else {
        // fp16 outputs: slab [64 m][64 n] halves, row stride 72 halves (144 B); 2 passes
        _Float16 *slab = smem + w * 8192;  // 16 KiB per wave
        constexpr int LS = 72;
        // EPI_QK: the scale (1/8 and log2 e on Q) applies to columns < scale_cols -- a multiple of 64, so a wave's 64 columns
        // are all in or all out (per element this was a compare, a select and a multiply on every output)
        const float qscale = (EPI == EPI_QK && nw0 < G.scale_cols) ? G.scale : 1.0f;
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            epi_sync();
            // per-lane row constants of the two 32-row blocks of this pass (FOLD: r and mu r of the token; tokens are the rows)
            float rs[2] = {1.f, 1.f}, mrs[2] = {0.f, 0.f};
            if constexpr (FOLD) {
#pragma unroll
                for (int yy = 0; yy < 2; ++yy) {
                    const float *sp = smem_f + EPB_OFF + EPB_STATS + 2 * (wm * 128 + (2 * p + yy) * 32 + i);
                    rs[yy] = sp[1];
                    mrs[yy] = sp[0] * sp[1];
                }
            }
#pragma unroll
            for (int x = 0; x < 2; ++x)
#pragma unroll
                for (int rq = 0; rq < 4; ++rq) {
                    const int nl = x * 32 + 8 * rq + 4 * g;  // local n of element 0
                    // column constants once per column quad (they come from LDS in the folded epilogues: one read per pass
                    // and quad instead of one per 32-row block)
                    f32x4 bias, cs = {0.f, 0.f, 0.f, 0.f};
                    if constexpr (FOLD) {
                        bias = *reinterpret_cast<const f32x4 *>(smem_f + EPB_OFF + EPB_VEC + wn * 64 + nl);
                        cs = *reinterpret_cast<const f32x4 *>(smem_f + EPB_OFF + EPB_VEC + 256 + wn * 64 + nl);
                    } else {
                        bias = *reinterpret_cast<const f32x4 *>(G.bias + nw0 + nl);
                    }
#pragma unroll
                    for (int yy = 0; yy < 2; ++yy) {
                        const f32x16 &a = acc[x][2 * p + yy];
                        f32x4 t = f32x4{a[4 * rq], a[4 * rq + 1], a[4 * rq + 2], a[4 * rq + 3]};
                        if constexpr (FOLD) t = t * rs[yy] + (bias - mrs[yy] * cs);  // r (acc - mu c) + b'
                        else t = t + bias;
                        if constexpr (EPI == EPI_GELU) {
                            t = gelu_erf256(t);
                        } else {
                            t = t * qscale;
                        }
                        const f16x4 v = f16x4{(_Float16)t[0], (_Float16)t[1], (_Float16)t[2], (_Float16)t[3]};
                        *reinterpret_cast<f16x4 *>(slab + (yy * 32 + i) * LS + nl) = v;
                    }
                }
            epi_sync();
            // read back: 8 lanes cover one row (64 halves = 128 B), 8 rows per instruction
            const int c8 = l & 7;
            _Float16 *po = G.out16 + (size_t)(mw0 + p * 64 + (l >> 3)) * G.ldc + nw0 + c8 * 8;  // running pointer: 8 rows per step
            const size_t ostep = (size_t)8 * G.ldc;
#pragma unroll
            for (int it = 0; it < 8; ++it) {
                const int rr = it * 8 + (l >> 3);
                const f16x8 v = *reinterpret_cast<const f16x8 *>(slab + rr * LS + c8 * 8);
                *reinterpret_cast<f16x8 *>(po + it * ostep) = v;
            }
        }
    }
}

}  // namespace ance
