// What the row-wise training kernels share (layer_tail.hip, layer_tail_half.hip, embed_train.hip): one wave owns a row and holds it in registers, lane l
// has the float4 at columns 4 (64 i + l), i < width / 256; the row sums are xor butterflies over the 64 lanes (every lane ends with
// the same bits).  A workgroup is four waves and owns LT_ROWS = 16 consecutive rows, four per wave.
// Column sums, without atomics: a wave adds its rows' terms per column in registers in ascending row order, the four waves meet in
// LDS as (w0 + w1) + (w2 + w3) and the workgroup writes ONE partial row (write_partial); colsum_tree_kernel sums the partial rows per
// column as a fixed binary tree whose shape depends on their number alone.  Every file that includes this gets its own copy of the
// kernel (an unnamed namespace): the same code, the same bits.  The host helpers behind them are inline: a file uses those it needs.
#pragma once
#include "common.h"

#include <stdio.h>

namespace ance {
namespace {

constexpr int LT_THREADS = 256, LT_WAVES = 4, LT_ROWS = ANCE_LAYER_TAIL_ROWS_PER_WORKGROUP, LT_RPW = LT_ROWS / LT_WAVES;
constexpr int CS_LEVELS = 21;  // the reducer's pairwise stack: a slice holds at most 2^20 groups of eight partials (n_part <= 2^27)
static_assert(LT_ROWS % LT_WAVES == 0, "a wave owns a whole number of rows");

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

__device__ __forceinline__ f32x4 load4(const float *p) { return *reinterpret_cast<const f32x4 *>(p); }
__device__ __forceinline__ void store4(float *p, const f32x4 v) { *reinterpret_cast<f32x4 *>(p) = v; }

template <int NV>
__device__ __forceinline__ void load_vec(f32x4 (&v)[NV], const float *p, int lane) {
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = p ? load4(p + 4 * (64 * i + lane)) : f32x4{0.f, 0.f, 0.f, 0.f};
}

// The four waves' per-column sums acc[NQ * NV] (float4 q * NV + i of lane l: column 4 (64 i + l) of quantity q) -> one partial row
// [NQ][256 NV] of this workgroup, summed (w0 + w1) + (w2 + w3).  sm: [2][NQ * NV * 64] float4.
template <int NA>
__device__ __forceinline__ void write_partial(f32x4 *sm, const f32x4 (&acc)[NA], float *part_row) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    f32x4 *mine = sm + (wave >> 1) * (NA * 64);
    if ((wave & 1) == 0) {
#pragma unroll
        for (int a = 0; a < NA; ++a) mine[a * 64 + lane] = acc[a];
    }
    __syncthreads();
    if (wave & 1) {
#pragma unroll
        for (int a = 0; a < NA; ++a) mine[a * 64 + lane] = mine[a * 64 + lane] + acc[a];
    }
    __syncthreads();
    for (int e = threadIdx.x; e < NA * 64; e += LT_THREADS) store4(part_row + 4 * e, sm[e] + sm[NA * 64 + e]);
}

// out_q[c] = sum over the n_part partial rows of part[p][q * hq + c], per 64-column group of the W = n_q * hq columns; 256 threads
// = 16 column quads x 16 slices of consecutive partial rows.  Every slice walks the same number of groups of eight (rows past n_part
// count as zeros), so the tree is a function of n_part alone.
__global__ void __launch_bounds__(256) colsum_tree_kernel(const float *part, int64_t n_part, int W, int hq, float *o0, float *o1, float *o2) {
    __shared__ __attribute__((aligned(16))) f32x4 sm[256];
    const int cq = threadIdx.x & 15, s = threadIdx.x >> 4;
    const int col = blockIdx.x * 64 + 4 * cq;
    const int64_t groups = ((n_part + 15) / 16 + 7) / 8, p0 = (int64_t)s * groups * 8;
    const f32x4 zero = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 st[CS_LEVELS];
#pragma unroll
    for (int l = 0; l < CS_LEVELS; ++l) st[l] = zero;
    for (int64_t g = 0; g < groups; ++g) {
        f32x4 v[8];
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const int64_t p = p0 + g * 8 + t;
            v[t] = p < n_part ? load4(part + p * W + col) : zero;
        }
        f32x4 x = ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
        // pairwise stack: level l holds the sum of 2^l groups while bit l of the number of groups pushed so far is set
        bool placed = false;
#pragma unroll
        for (int l = 0; l < CS_LEVELS; ++l) {
            if (!placed) {
                if ((g >> l) & 1) {
                    x = st[l] + x;
                } else {
                    st[l] = x;
                    placed = true;
                }
            }
        }
    }
    f32x4 r = zero;
    bool have = false;
#pragma unroll
    for (int l = 0; l < CS_LEVELS; ++l) {
        if ((groups >> l) & 1) {
            r = have ? st[l] + r : st[l];
            have = true;
        }
    }
    sm[threadIdx.x] = r;
    __syncthreads();
#pragma unroll
    for (int half = 8; half > 0; half >>= 1) {
        if (s < half) sm[threadIdx.x] = sm[threadIdx.x] + sm[threadIdx.x + 16 * half];
        __syncthreads();
    }
    if (s == 0) {
        const int q = col / hq;
        float *o = q == 0 ? o0 : (q == 1 ? o1 : o2);
        if (o) store4(o + (col - q * hq), sm[threadIdx.x]);
    }
}

inline bool rows_ok(int64_t n_rows) { return n_rows >= 1 && n_rows <= 0x7fffffff; }
inline size_t n_part(int64_t n_rows) { return (size_t)((n_rows + LT_ROWS - 1) / LT_ROWS); }
inline size_t stats_bytes(int64_t n_rows) { return 2 * align_up(sizeof(float) * (size_t)n_rows, 256); }

inline const char *check_matrix(const void *p, int ld, int width, bool nullable = false) {
    if (!p) return nullable ? nullptr : "null pointer";
    if ((uintptr_t)p % 16) return "alignment: a base is not 16-byte aligned";
    if (ld % 4 != 0 || ld < width) return "stride: not a multiple of 4 or below the width";
    return nullptr;
}
inline const char *check_vector(const void *p, bool nullable = false) {
    if (!p) return nullable ? nullptr : "null pointer";
    if ((uintptr_t)p % 16) return "alignment: a base is not 16-byte aligned";
    return nullptr;
}
inline const char *check_workspace(const void *p, size_t have, size_t need) {
    if (!p || (uintptr_t)p % 16) return "null or unaligned workspace";
    if (have < need) return "workspace too small";
    return nullptr;
}

}  // namespace
}  // namespace ance
