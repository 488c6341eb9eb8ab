// The kernels of the BertLayer's row-wise seams, once, for both precisions of their matmul-side I/O (layer_tail.hip: X = F32, fp32
// throughout; layer_tail_half.hip: X = F16 / BF16, 16-bit x / dx / y16 / dy16 around an fp32 residual stream), behind the one host
// front end of layer_tail_common.h, which fills the parameter blocks and picks X at the launch.  The arithmetic behind
// the load and in front of the store is one text, so on an x that holds 16-bit values the 16-bit tail's fp32 outputs are the fp32
// tail's bits.  The organisation (one wave per row, lane l at columns 4 (64 i + l) .. + 3, 16 rows per workgroup, partial rows, the
// column-sum tree) is row_kernels.h's; the contracts are include/ance_amd.h's.
// X names the element type T of the matmul-side rows and the parameter blocks of its kernels.  With T = float a lane's piece of a
// row is 16 bytes; with a 16-bit T it is 8 bytes (512 B contiguous per wave) next to the 16 bytes of the fp32 rows: 768 / 64 lanes
// = 12 halves = 24 bytes, so 16 bytes per lane of a 16-bit row do not divide the tail's widths, and this layout keeps one Philox
// call per four columns, the wave reductions and write_partial as they are.  Rounding to a 16-bit T is the compiler's conversion:
// to nearest even, +-inf on overflow, never clamped.
#pragma once
#include "common.h"
#include "philox.h"
#include "row_kernels.h"

#include <math.h>

namespace ance {
namespace {

struct TailParams {
    const float *x, *res, *bias, *gamma, *beta, *dy;
    float *y, *dx, *dres;
    int64_t ld_x, ld_res, ld_y, ld_dy, ld_dx, ld_dres;
    int64_t n_rows;
    float *mean, *rstd, *part;
    float eps, keep_scale;
    uint32_t seed_lo, seed_hi, off_lo, off_hi, keep_thr;
    const uint64_t *d_stream;  // null, or the device stream {seed, base} (philox.h: drop_stream)
};

struct GeluParams {
    const float *x, *bias, *dy;
    float *y, *dx, *part;
    int64_t ld_x, ld_y, ld_dy, ld_dx;
    int64_t n_rows;
};

// x, y16, dy16, dx are T rows; dy (fp32) and dy16 are each optional, one is given: g = dy + float(dy16) in registers
struct TailParams16 {
    const void *x, *dy16;
    const float *res, *bias, *gamma, *beta, *dy;
    float *y, *dres;
    void *y16, *dx;
    int64_t ld_x, ld_res, ld_y, ld_y16, ld_dy, ld_dy16, ld_dx, ld_dres;
    int64_t n_rows;
    float *mean, *rstd, *part;
    float eps, keep_scale;
    uint32_t seed_lo, seed_hi, off_lo, off_hi, keep_thr;
    const uint64_t *d_stream;  // null, or the device stream {seed, base} (philox.h: drop_stream)
};

struct GeluParams16 {
    const void *x, *dy;
    const float *bias;
    void *y, *dx;
    float *part;
    int64_t ld_x, ld_y, ld_dy, ld_dx;
    int64_t n_rows;
};

struct F32 {
    typedef float T;
    typedef f32x4 V4;
    typedef TailParams Tail;
    typedef GeluParams Gelu;
    static constexpr bool HALF = false;
};
struct F16 {
    typedef _Float16 T;
    typedef _Float16 V4 __attribute__((ext_vector_type(4)));
    typedef TailParams16 Tail;
    typedef GeluParams16 Gelu;
    static constexpr bool HALF = true;
};
struct BF16 {
    typedef __bf16 T;
    typedef __bf16 V4 __attribute__((ext_vector_type(4)));
    typedef TailParams16 Tail;
    typedef GeluParams16 Gelu;
    static constexpr bool HALF = true;
};

// a parameter block's pointer as T rows; four consecutive T elements as floats, and back (rounded once)
template <class X>
__device__ __forceinline__ const typename X::T *rows_t(const void *base) { return reinterpret_cast<const typename X::T *>(base); }
template <class X>
__device__ __forceinline__ typename X::T *rows_t(void *base) { return reinterpret_cast<typename X::T *>(base); }
template <class X>
__device__ __forceinline__ f32x4 load4_t(const typename X::T *p) {
    const typename X::V4 h = *reinterpret_cast<const typename X::V4 *>(p);
    if constexpr (X::HALF) return f32x4{(float)h[0], (float)h[1], (float)h[2], (float)h[3]};
    else return h;
}
template <class X>
__device__ __forceinline__ void store4_t(typename X::T *p, const f32x4 v) {
    typedef typename X::T T;
    if constexpr (X::HALF) *reinterpret_cast<typename X::V4 *>(p) = typename X::V4{(T)v[0], (T)v[1], (T)v[2], (T)v[3]};
    else *reinterpret_cast<typename X::V4 *>(p) = v;
}

// z = keep o (x + bias) / (1 - p) + res of one row under the stream D (resolved once at kernel entry), and the row's keep bits (bit e of keep[i]: column 4 (64 i + lane) + e).  The
// forward and the backward both come through here, with contraction off: the same bits both times.
template <class X, int NV, int DROP>
__device__ __forceinline__ void tail_z(const typename X::Tail &P, const DropStream &D, int64_t row, int lane, const f32x4 (&b)[NV], f32x4 (&z)[NV], uint32_t (&keep)[NV]) {
#pragma clang fp contract(off)
    const typename X::T *xr = rows_t<X>(P.x) + row * P.ld_x;
    const float *rr = P.res + row * P.ld_res;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c4 = 64 * i + lane;
        f32x4 u = load4_t<X>(xr + 4 * c4) + b[i];
        const f32x4 r = load4(rr + 4 * c4);
        keep[i] = 0xfu;
        if (DROP) {
            uint32_t w[4];
            philox4((uint32_t)row, (uint32_t)c4, D.off_lo, D.off_hi, D.seed_lo, D.seed_hi, w);
            keep[i] = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const bool k = w[e] >= P.keep_thr;
                u[e] = k ? u[e] * P.keep_scale : 0.f;
                keep[i] |= (k ? 1u : 0u) << e;
            }
        }
        z[i] = u + r;
    }
}

template <class X, int NV, int DROP>
__global__ void __launch_bounds__(LT_THREADS) tail_fwd_kernel(const typename X::Tail P) {
    const DropStream D = drop_stream<DROP>(P);
    constexpr float H = (float)(256 * NV);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    f32x4 b[NV], ga[NV], be[NV];
    load_vec(b, P.bias, lane);
    load_vec(ga, P.gamma, lane);
    load_vec(be, P.beta, lane);
    const int64_t r0 = (int64_t)blockIdx.x * LT_ROWS + wave * LT_RPW;
    for (int j = 0; j < LT_RPW; ++j) {
        const int64_t row = r0 + j;
        if (row >= P.n_rows) break;  // the same in every lane of the wave
        f32x4 z[NV];
        uint32_t keep[NV];
        tail_z<X, NV, DROP>(P, D, row, lane, b, z, keep);
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < NV; ++i) s += (z[i][0] + z[i][1]) + (z[i][2] + z[i][3]);
        const float mean = wave_sum(s) / H;
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            z[i] -= mean;
            q += (z[i][0] * z[i][0] + z[i][1] * z[i][1]) + (z[i][2] * z[i][2] + z[i][3] * z[i][3]);
        }
        const float rstd = 1.0f / sqrtf(wave_sum(q) / H + P.eps);
        float *yr = P.y + row * P.ld_y;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const f32x4 o = z[i] * rstd * ga[i] + be[i];
            store4(yr + 4 * (64 * i + lane), o);
            if constexpr (X::HALF) {
                if (P.y16) store4_t<X>(rows_t<X>(P.y16) + row * P.ld_y16 + 4 * (64 * i + lane), o);  // the same registers, rounded once
            }
        }
        if (lane == 0) {
            P.mean[row] = mean;
            P.rstd[row] = rstd;
        }
    }
}

template <class X, int NV, int DROP>
__global__ void __launch_bounds__(LT_THREADS) tail_bwd_kernel(const typename X::Tail P) {
    const DropStream D = drop_stream<DROP>(P);
    __shared__ __attribute__((aligned(16))) f32x4 sm[2 * 3 * NV * 64];
    constexpr float H = (float)(256 * NV);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    f32x4 b[NV], ga[NV];
    load_vec(b, P.bias, lane);
    load_vec(ga, P.gamma, lane);
    f32x4 acc[3 * NV];  // dgamma, dbeta, dbias
#pragma unroll
    for (int a = 0; a < 3 * NV; ++a) acc[a] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int64_t r0 = (int64_t)blockIdx.x * LT_ROWS + wave * LT_RPW;
    for (int j = 0; j < LT_RPW; ++j) {
        const int64_t row = r0 + j;
        if (row >= P.n_rows) break;  // the same in every lane of the wave
        f32x4 xh[NV], g[NV];
        uint32_t keep[NV];
        tail_z<X, NV, DROP>(P, D, row, lane, b, xh, keep);
        const float mean = P.mean[row], rstd = P.rstd[row];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            f32x4 dy;
            if constexpr (X::HALF) {  // the residual's fp32 gradient plus the Linears' 16-bit one, whichever exist
                if (P.dy) {
                    dy = load4(P.dy + row * P.ld_dy + 4 * (64 * i + lane));
                    if (P.dy16) dy = dy + load4_t<X>(rows_t<X>(P.dy16) + row * P.ld_dy16 + 4 * (64 * i + lane));
                } else {
                    dy = load4_t<X>(rows_t<X>(P.dy16) + row * P.ld_dy16 + 4 * (64 * i + lane));
                }
            } else {
                const float *gr = P.dy + row * P.ld_dy;
                dy = load4(gr + 4 * (64 * i + lane));
            }
            xh[i] = (xh[i] - mean) * rstd;
            g[i] = dy * ga[i];
            const f32x4 gx = g[i] * xh[i];
            s1 += (g[i][0] + g[i][1]) + (g[i][2] + g[i][3]);
            s2 += (gx[0] + gx[1]) + (gx[2] + gx[3]);
            acc[i] += dy * xh[i];
            acc[NV + i] += dy;
        }
        const float m1 = wave_sum(s1) / H, m2 = wave_sum(s2) / H;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const f32x4 dz = (g[i] - m1 - xh[i] * m2) * rstd;
            f32x4 dx = dz;
            if (DROP) {
#pragma unroll
                for (int e = 0; e < 4; ++e) dx[e] = (keep[i] >> e) & 1u ? dz[e] * P.keep_scale : 0.f;
            }
            if (P.dres) store4(P.dres + row * P.ld_dres + 4 * (64 * i + lane), dz);
            if (P.dx) store4_t<X>(rows_t<X>(P.dx) + row * P.ld_dx + 4 * (64 * i + lane), dx);
            acc[2 * NV + i] += dx;  // dbias sums the unrounded terms
        }
    }
    write_partial(sm, acc, P.part + (int64_t)blockIdx.x * (3 * 256 * NV));
}

constexpr float INV_SQRT2 = 0.70710678118654752440f, INV_SQRT_2PI = 0.39894228040143267794f;

template <class X, int NV>
__global__ void __launch_bounds__(LT_THREADS) gelu_fwd_kernel(const typename X::Gelu P) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    f32x4 b[NV];
    load_vec(b, P.bias, lane);
    const int64_t r0 = (int64_t)blockIdx.x * LT_ROWS + wave * LT_RPW;
    for (int j = 0; j < LT_RPW; ++j) {
        const int64_t row = r0 + j;
        if (row >= P.n_rows) break;
        const typename X::T *xr = rows_t<X>(P.x) + row * P.ld_x;
        typename X::T *yr = rows_t<X>(P.y) + row * P.ld_y;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const f32x4 u = load4_t<X>(xr + 4 * (64 * i + lane)) + b[i];
            f32x4 y;
#pragma unroll
            for (int e = 0; e < 4; ++e) y[e] = 0.5f * u[e] * (1.0f + erff(u[e] * INV_SQRT2));
            store4_t<X>(yr + 4 * (64 * i + lane), y);
        }
    }
}

template <class X, int NV>
__global__ void __launch_bounds__(LT_THREADS) gelu_bwd_kernel(const typename X::Gelu P) {
    __shared__ __attribute__((aligned(16))) f32x4 sm[2 * NV * 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    f32x4 b[NV], acc[NV];
    load_vec(b, P.bias, lane);
#pragma unroll
    for (int i = 0; i < NV; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int64_t r0 = (int64_t)blockIdx.x * LT_ROWS + wave * LT_RPW;
    for (int j = 0; j < LT_RPW; ++j) {
        const int64_t row = r0 + j;
        if (row >= P.n_rows) break;
        const typename X::T *xr = rows_t<X>(P.x) + row * P.ld_x, *gr = rows_t<X>(P.dy) + row * P.ld_dy;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const f32x4 u = load4_t<X>(xr + 4 * (64 * i + lane)) + b[i], dy = load4_t<X>(gr + 4 * (64 * i + lane));
            f32x4 dx;
#pragma unroll
            for (int e = 0; e < 4; ++e)
                dx[e] = dy[e] * (0.5f * (1.0f + erff(u[e] * INV_SQRT2)) + u[e] * expf(-0.5f * u[e] * u[e]) * INV_SQRT_2PI);
            if (P.dx) store4_t<X>(rows_t<X>(P.dx) + row * P.ld_dx + 4 * (64 * i + lane), dx);
            acc[i] += dx;  // dbias sums the unrounded terms
        }
    }
    write_partial(sm, acc, P.part + (int64_t)blockIdx.x * (256 * NV));
}

// the launches, by width and by how the masks are drawn (philox.h: drop_mode)
template <class X, int DROP>
void launch_tail_fwd_as(int H, dim3 grid, hipStream_t st, const typename X::Tail &P) {
    const dim3 block(LT_THREADS);
    if (H == 768) hipLaunchKernelGGL((tail_fwd_kernel<X, 3, DROP>), grid, block, 0, st, P);
    else hipLaunchKernelGGL((tail_fwd_kernel<X, 4, DROP>), grid, block, 0, st, P);
}
template <class X>
void launch_tail_fwd(int H, bool drop, dim3 grid, hipStream_t st, const typename X::Tail &P) {
    const int mode = drop_mode(drop, P.d_stream);
    if (mode == DROP_DEVICE) launch_tail_fwd_as<X, DROP_DEVICE>(H, grid, st, P);
    else if (mode == DROP_HOST) launch_tail_fwd_as<X, DROP_HOST>(H, grid, st, P);
    else launch_tail_fwd_as<X, DROP_NONE>(H, grid, st, P);
}
template <class X, int DROP>
void launch_tail_bwd_as(int H, dim3 grid, hipStream_t st, const typename X::Tail &P) {
    const dim3 block(LT_THREADS);
    if (H == 768) hipLaunchKernelGGL((tail_bwd_kernel<X, 3, DROP>), grid, block, 0, st, P);
    else hipLaunchKernelGGL((tail_bwd_kernel<X, 4, DROP>), grid, block, 0, st, P);
}
template <class X>
void launch_tail_bwd(int H, bool drop, dim3 grid, hipStream_t st, const typename X::Tail &P) {
    const int mode = drop_mode(drop, P.d_stream);
    if (mode == DROP_DEVICE) launch_tail_bwd_as<X, DROP_DEVICE>(H, grid, st, P);
    else if (mode == DROP_HOST) launch_tail_bwd_as<X, DROP_HOST>(H, grid, st, P);
    else launch_tail_bwd_as<X, DROP_NONE>(H, grid, st, P);
}
template <class X>
void launch_gelu_fwd(int N, dim3 grid, hipStream_t st, const typename X::Gelu &P) {
    if (N == 3072) hipLaunchKernelGGL((gelu_fwd_kernel<X, 12>), grid, dim3(LT_THREADS), 0, st, P);
    else hipLaunchKernelGGL((gelu_fwd_kernel<X, 16>), grid, dim3(LT_THREADS), 0, st, P);
}
template <class X>
void launch_gelu_bwd(int N, dim3 grid, hipStream_t st, const typename X::Gelu &P) {
    if (N == 3072) hipLaunchKernelGGL((gelu_bwd_kernel<X, 12>), grid, dim3(LT_THREADS), 0, st, P);
    else hipLaunchKernelGGL((gelu_bwd_kernel<X, 16>), grid, dim3(LT_THREADS), 0, st, P);
}

// the column-sum launches behind the two backward row kernels
inline void launch_tail_colsum(const float *part, int64_t n_rows, int H, float *dgamma, float *dbeta, float *dbias, hipStream_t st) {
    hipLaunchKernelGGL(colsum_tree_kernel, dim3((unsigned)(3 * H / 64)), dim3(256), 0, st, part, (int64_t)n_part(n_rows), 3 * H, H, dgamma,
                       dbeta, dbias);
}
inline void launch_gelu_colsum(const float *part, int64_t n_rows, int N, float *dbias, hipStream_t st) {
    hipLaunchKernelGGL(colsum_tree_kernel, dim3((unsigned)(N / 64)), dim3(256), 0, st, part, (int64_t)n_part(n_rows), N, N, dbias,
                       (float *)nullptr, (float *)nullptr);
}

inline size_t tail_ws_bytes(int64_t n_rows, int H) { return stats_bytes(n_rows) + n_part(n_rows) * 3 * (size_t)H * sizeof(float); }
inline size_t gelu_ws_bytes(int64_t n_rows, int N) { return n_part(n_rows) * (size_t)N * sizeof(float); }

}  // namespace
}  // namespace ance
