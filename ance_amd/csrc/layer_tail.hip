// The row-wise seams of a BertLayer with their gradients (include/ance_amd.h: ance_layer_tail_* and ance_bias_gelu_*): what
// transformers' eager BertSelfOutput / BertOutput compute after their dense matmul, and BertIntermediate after its own.
//   tail   u = x + bias;  d = keep o u / (1 - p) (training, p > 0), else u;  z = d + res;  y = LayerNorm(z) gamma + beta
//          mean = sum z / H, var = sum (z - mean)^2 / H over the row held in registers (two passes, biased), rstd = 1 / sqrtf(var + eps)
//          backward: xhat recomputed from x, bias, res, the regenerated mask and the saved (mean, rstd);  g = dy o gamma;
//          dz = rstd (g - mean_H(g) - xhat mean_H(g o xhat));  dres = dz;  dx = keep o dz / (1 - p);
//          dgamma = sum_r dy o xhat, dbeta = sum_r dy, dbias = sum_r dx
//   gelu   u = x + bias;  y = 0.5 u (1 + erff(u / sqrt 2));  dx = dy (0.5 (1 + erff(u / sqrt 2)) + u expf(-u^2 / 2) / sqrt(2 pi));
//          dbias = sum_r dx
// One wave owns a row and holds it in registers: lane l has the float4 at columns 4 (64 i + l), i < width / 256, so every load and
// store is 16 bytes per lane and 1 KiB contiguous per wave; the row sums are xor butterflies over the 64 lanes (every lane ends with
// the same bits).  A workgroup is four waves and owns LT_ROWS = 16 consecutive rows, four per wave.
// Column sums, without atomics: a wave adds its rows' terms per column in registers in ascending row order, the four waves meet in
// LDS as (w0 + w1) + (w2 + w3), and the workgroup writes ONE partial row into the workspace ([n_part][3][H] for the tail: dgamma,
// dbeta, dbias; [n_part][N] for the GELU), n_part = ceil(n_rows / 16).  The second launch sums the partial rows per column as a fixed
// binary tree: sixteen slices of consecutive partials, each slice a pairwise tree over groups of eight (the groups themselves summed
// ((0+1)+(2+3))+((4+5)+(6+7))), the slices met in LDS by halving.  Its shape depends on n_part alone: the same inputs give the same bits.
// Dropout: Philox4x32-10, key (seed lo, seed hi), counter (row, col >> 2, offset lo, offset hi), word col & 3 decides column col: one
// call per float4; keep iff word >= floor(p 2^32).
// The row reductions, the partial rows, the column-sum tree and the argument checks are row_kernels.h's, shared with embed_train.hip.
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
};

struct GeluParams {
    const float *x, *bias, *dy;
    float *y, *dx, *part;
    int64_t ld_x, ld_y, ld_dy, ld_dx;
    int64_t n_rows;
};

// z = keep o (x + bias) / (1 - p) + res of one row, and the row's keep bits (bit e of keep[i]: column 4 (64 i + lane) + e).  The
// forward and the backward both come through here, with contraction off: the same bits both times.
template <int NV, bool DROP>
__device__ __forceinline__ void tail_z(const TailParams &P, int64_t row, int lane, const f32x4 (&b)[NV], f32x4 (&z)[NV], uint32_t (&keep)[NV]) {
#pragma clang fp contract(off)
    const float *xr = P.x + row * P.ld_x, *rr = P.res + row * P.ld_res;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c4 = 64 * i + lane;
        f32x4 u = load4(xr + 4 * c4) + b[i];
        const f32x4 r = load4(rr + 4 * c4);
        keep[i] = 0xfu;
        if (DROP) {
            uint32_t w[4];
            philox4((uint32_t)row, (uint32_t)c4, P.off_lo, P.off_hi, P.seed_lo, P.seed_hi, w);
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

template <int NV, bool DROP>
__global__ void __launch_bounds__(LT_THREADS) tail_fwd_kernel(const TailParams P) {
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
        tail_z<NV, DROP>(P, row, lane, b, z, keep);
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
        for (int i = 0; i < NV; ++i) store4(yr + 4 * (64 * i + lane), z[i] * rstd * ga[i] + be[i]);
        if (lane == 0) {
            P.mean[row] = mean;
            P.rstd[row] = rstd;
        }
    }
}

template <int NV, bool DROP>
__global__ void __launch_bounds__(LT_THREADS) tail_bwd_kernel(const TailParams P) {
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
        tail_z<NV, DROP>(P, row, lane, b, xh, keep);
        const float mean = P.mean[row], rstd = P.rstd[row];
        const float *gr = P.dy + row * P.ld_dy;
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const f32x4 dy = load4(gr + 4 * (64 * i + lane));
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
            if (P.dx) store4(P.dx + row * P.ld_dx + 4 * (64 * i + lane), dx);
            acc[2 * NV + i] += dx;
        }
    }
    write_partial(sm, acc, P.part + (int64_t)blockIdx.x * (3 * 256 * NV));
}

constexpr float INV_SQRT2 = 0.70710678118654752440f, INV_SQRT_2PI = 0.39894228040143267794f;

template <int NV>
__global__ void __launch_bounds__(LT_THREADS) gelu_fwd_kernel(const GeluParams P) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    f32x4 b[NV];
    load_vec(b, P.bias, lane);
    const int64_t r0 = (int64_t)blockIdx.x * LT_ROWS + wave * LT_RPW;
    for (int j = 0; j < LT_RPW; ++j) {
        const int64_t row = r0 + j;
        if (row >= P.n_rows) break;
        const float *xr = P.x + row * P.ld_x;
        float *yr = P.y + row * P.ld_y;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const f32x4 u = load4(xr + 4 * (64 * i + lane)) + b[i];
            f32x4 y;
#pragma unroll
            for (int e = 0; e < 4; ++e) y[e] = 0.5f * u[e] * (1.0f + erff(u[e] * INV_SQRT2));
            store4(yr + 4 * (64 * i + lane), y);
        }
    }
}

template <int NV>
__global__ void __launch_bounds__(LT_THREADS) gelu_bwd_kernel(const GeluParams P) {
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
        const float *xr = P.x + row * P.ld_x, *gr = P.dy + row * P.ld_dy;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const f32x4 u = load4(xr + 4 * (64 * i + lane)) + b[i], dy = load4(gr + 4 * (64 * i + lane));
            f32x4 dx;
#pragma unroll
            for (int e = 0; e < 4; ++e)
                dx[e] = dy[e] * (0.5f * (1.0f + erff(u[e] * INV_SQRT2)) + u[e] * expf(-0.5f * u[e] * u[e]) * INV_SQRT_2PI);
            if (P.dx) store4(P.dx + row * P.ld_dx + 4 * (64 * i + lane), dx);
            acc[i] += dx;
        }
    }
    write_partial(sm, acc, P.part + (int64_t)blockIdx.x * (256 * NV));
}

size_t tail_ws_bytes(int64_t n_rows, int H) { return stats_bytes(n_rows) + n_part(n_rows) * 3 * (size_t)H * sizeof(float); }
size_t gelu_ws_bytes(int64_t n_rows, int N) { return n_part(n_rows) * (size_t)N * sizeof(float); }

const char *check_tail(const AnceLayerTailArgs *a, bool backward) {
    if (!a) return "null pointer";
    if (a->H != 768 && a->H != 1024) return "width H not 768 or 1024";
    if (a->n_rows < 1) return "n_rows < 1";
    if (const char *why = check_matrix(a->x, a->ld_x, a->H)) return why;
    if (const char *why = check_matrix(a->res, a->ld_res, a->H)) return why;
    if (const char *why = check_vector(a->bias, true)) return why;
    if (const char *why = check_vector(a->gamma)) return why;
    if (!backward) {  // the backward touches neither y nor beta
        if (const char *why = check_matrix(a->y, a->ld_y, a->H)) return why;
        if (const char *why = check_vector(a->beta)) return why;
    }
    if (!(a->dropout_p >= 0.0f && a->dropout_p < 1.0f)) return "dropout_p outside [0, 1)";
    if (!(a->eps > 0.0f)) return "eps <= 0";
    return check_workspace(a->d_workspace, a->workspace_bytes, backward ? tail_ws_bytes(a->n_rows, a->H) : stats_bytes(a->n_rows));
}
TailParams tail_params(const AnceLayerTailArgs *a) {
    TailParams P = {};
    P.x = a->x; P.res = a->res; P.bias = a->bias; P.gamma = a->gamma; P.beta = a->beta; P.y = a->y;
    P.ld_x = a->ld_x; P.ld_res = a->ld_res; P.ld_y = a->ld_y;
    P.n_rows = a->n_rows;
    P.mean = (float *)a->d_workspace;
    P.rstd = (float *)((char *)a->d_workspace + stats_bytes(a->n_rows) / 2);
    P.part = (float *)((char *)a->d_workspace + stats_bytes(a->n_rows));
    P.eps = a->eps;
    P.seed_lo = (uint32_t)a->seed; P.seed_hi = (uint32_t)(a->seed >> 32);
    P.off_lo = (uint32_t)a->offset; P.off_hi = (uint32_t)(a->offset >> 32);
    P.keep_thr = (uint32_t)((double)a->dropout_p * 4294967296.0);  // floor(p 2^32), p < 1
    P.keep_scale = 1.0f / (1.0f - a->dropout_p);
    return P;
}
bool drops(const AnceLayerTailArgs *a) { return a->training != 0 && a->dropout_p > 0.0f; }

const char *check_gelu(const AnceBiasGeluArgs *a, bool backward) {
    if (!a) return "null pointer";
    if (a->N != 3072 && a->N != 4096) return "width N not 3072 or 4096";
    if (a->n_rows < 1) return "n_rows < 1";
    if (const char *why = check_matrix(a->x, a->ld_x, a->N)) return why;
    if (!backward) {  // the backward does not touch y
        if (const char *why = check_matrix(a->y, a->ld_y, a->N)) return why;
    }
    return check_vector(a->bias);
}
GeluParams gelu_params(const AnceBiasGeluArgs *a) {
    GeluParams P = {};
    P.x = a->x; P.bias = a->bias; P.y = a->y;
    P.ld_x = a->ld_x; P.ld_y = a->ld_y;
    P.n_rows = a->n_rows;
    P.part = (float *)a->d_workspace;
    return P;
}

}  // namespace
}  // namespace ance

extern "C" int ance_layer_tail_rows_per_workgroup(void) { return ance::LT_ROWS; }

extern "C" size_t ance_layer_tail_workspace_bytes(int64_t n_rows, int H) {
    using namespace ance;
    return rows_ok(n_rows) && (H == 768 || H == 1024) ? tail_ws_bytes(n_rows, H) : 0;
}

extern "C" size_t ance_bias_gelu_workspace_bytes(int64_t n_rows, int N) {
    using namespace ance;
    return rows_ok(n_rows) && (N == 3072 || N == 4096) ? gelu_ws_bytes(n_rows, N) : 0;
}

extern "C" int ance_layer_tail_forward(const AnceLayerTailArgs *args, void *stream) {
    using namespace ance;
    const char *fn = "ance_layer_tail_forward";
    if (const char *why = check_tail(args, false)) return refuse(fn, why);
    const TailParams P = tail_params(args);
    const dim3 grid((unsigned)n_part(args->n_rows)), block(LT_THREADS);
    hipStream_t st = (hipStream_t)stream;
    const bool drop = drops(args);
    if (args->H == 768) {
        if (drop) hipLaunchKernelGGL((tail_fwd_kernel<3, true>), grid, block, 0, st, P);
        else hipLaunchKernelGGL((tail_fwd_kernel<3, false>), grid, block, 0, st, P);
    } else {
        if (drop) hipLaunchKernelGGL((tail_fwd_kernel<4, true>), grid, block, 0, st, P);
        else hipLaunchKernelGGL((tail_fwd_kernel<4, false>), grid, block, 0, st, P);
    }
    return check_launch(fn);
}

extern "C" int ance_layer_tail_backward(const AnceLayerTailArgs *args, const AnceLayerTailGradArgs *grads, void *stream) {
    using namespace ance;
    const char *fn = "ance_layer_tail_backward";
    if (const char *why = check_tail(args, true)) return refuse(fn, why);
    if (!grads) return refuse(fn, "null pointer");
    if (const char *why = check_matrix(grads->dy, grads->ld_dy, args->H)) return refuse(fn, why);
    if (const char *why = check_matrix(grads->dx, grads->ld_dx, args->H, true)) return refuse(fn, why);
    if (const char *why = check_matrix(grads->dres, grads->ld_dres, args->H, true)) return refuse(fn, why);
    if (const char *why = check_vector(grads->dgamma, true)) return refuse(fn, why);
    if (const char *why = check_vector(grads->dbeta, true)) return refuse(fn, why);
    if (const char *why = check_vector(grads->dbias, true)) return refuse(fn, why);
    TailParams P = tail_params(args);
    P.dy = grads->dy; P.dx = grads->dx; P.dres = grads->dres;
    P.ld_dy = grads->ld_dy; P.ld_dx = grads->ld_dx; P.ld_dres = grads->ld_dres;
    const dim3 grid((unsigned)n_part(args->n_rows)), block(LT_THREADS);
    hipStream_t st = (hipStream_t)stream;
    const bool drop = drops(args);
    if (args->H == 768) {
        if (drop) hipLaunchKernelGGL((tail_bwd_kernel<3, true>), grid, block, 0, st, P);
        else hipLaunchKernelGGL((tail_bwd_kernel<3, false>), grid, block, 0, st, P);
    } else {
        if (drop) hipLaunchKernelGGL((tail_bwd_kernel<4, true>), grid, block, 0, st, P);
        else hipLaunchKernelGGL((tail_bwd_kernel<4, false>), grid, block, 0, st, P);
    }
    float *dbias = args->bias ? grads->dbias : nullptr;  // no bias: no dbias
    hipLaunchKernelGGL(colsum_tree_kernel, dim3((unsigned)(3 * args->H / 64)), dim3(256), 0, st, (const float *)P.part,
                       (int64_t)n_part(args->n_rows), 3 * args->H, args->H, grads->dgamma, grads->dbeta, dbias);
    return check_launch(fn);
}

extern "C" int ance_bias_gelu_forward(const AnceBiasGeluArgs *args, void *stream) {
    using namespace ance;
    const char *fn = "ance_bias_gelu_forward";
    if (const char *why = check_gelu(args, false)) return refuse(fn, why);
    const GeluParams P = gelu_params(args);
    const dim3 grid((unsigned)n_part(args->n_rows)), block(LT_THREADS);
    hipStream_t st = (hipStream_t)stream;
    if (args->N == 3072) hipLaunchKernelGGL(gelu_fwd_kernel<12>, grid, block, 0, st, P);
    else hipLaunchKernelGGL(gelu_fwd_kernel<16>, grid, block, 0, st, P);
    return check_launch(fn);
}

extern "C" int ance_bias_gelu_backward(const AnceBiasGeluArgs *args, const AnceBiasGeluGradArgs *grads, void *stream) {
    using namespace ance;
    const char *fn = "ance_bias_gelu_backward";
    if (const char *why = check_gelu(args, true)) return refuse(fn, why);
    if (const char *why = check_workspace(args->d_workspace, args->workspace_bytes, gelu_ws_bytes(args->n_rows, args->N))) return refuse(fn, why);
    if (!grads) return refuse(fn, "null pointer");
    if (const char *why = check_matrix(grads->dy, grads->ld_dy, args->N)) return refuse(fn, why);
    if (const char *why = check_matrix(grads->dx, grads->ld_dx, args->N, true)) return refuse(fn, why);
    if (const char *why = check_vector(grads->dbias, true)) return refuse(fn, why);
    GeluParams P = gelu_params(args);
    P.dy = grads->dy; P.dx = grads->dx;
    P.ld_dy = grads->ld_dy; P.ld_dx = grads->ld_dx;
    const dim3 grid((unsigned)n_part(args->n_rows)), block(LT_THREADS);
    hipStream_t st = (hipStream_t)stream;
    if (args->N == 3072) hipLaunchKernelGGL(gelu_bwd_kernel<12>, grid, block, 0, st, P);
    else hipLaunchKernelGGL(gelu_bwd_kernel<16>, grid, block, 0, st, P);
    hipLaunchKernelGGL(colsum_tree_kernel, dim3((unsigned)(args->N / 64)), dim3(256), 0, st, (const float *)P.part,
                       (int64_t)n_part(args->n_rows), args->N, args->N, grads->dbias, (float *)nullptr, (float *)nullptr);
    return check_launch(fn);
}
