// The host front end of the BertLayer's row-wise seams, once for both entry families (layer_tail.hip: ance_layer_tail_* /
// ance_bias_gelu_*, fp32 throughout; layer_tail_half.hip: ance_layer_tail16_* / ance_bias_gelu16_*): one argument check, one
// parameter fill and one call skeleton per seam and direction over AnceLayerTail16Args / AnceBiasGelu16Args and their gradient
// structs, the internal form of every entry point (the fp32 entry points convert their structs once: dtype ANCE_DTYPE_F32, no y16 /
// dy16).  What a family accepts beyond the common rules is its dtype mask DTYPES (bit 1 << ANCE_DTYPE_*): the dtype of a call picks
// the 16-byte-piece rule of its T rows and, at the launch, the kernels' X and its parameter block -- and only the X of the family's
// mask are instantiated, so each file holds the kernels it held before.
#pragma once
#include "layer_tail_kernels.h"

namespace ance {
namespace {

constexpr unsigned ONLY_F32 = 1u << ANCE_DTYPE_F32, ONLY_16 = 1u << ANCE_DTYPE_F16 | 1u << ANCE_DTYPE_BF16;
// the fp32 family's dtype is set by its conversion and cannot miss
inline const char *check_dtype(int dtype, unsigned dtypes) {
    return dtype >= 0 && dtype <= 31 && (dtypes >> dtype & 1u) ? nullptr : "dtype neither ANCE_DTYPE_F16 nor ANCE_DTYPE_BF16";
}

// check_matrix for a T matrix: 16-byte pieces, so a row stride is a multiple of 4 floats (row_kernels.h) or of 8 16-bit elements
inline const char *check_matrix_t(int dtype, const void *p, int ld, int width, bool nullable = false) {
    if (dtype == ANCE_DTYPE_F32) return check_matrix(p, ld, width, nullable);
    if (!p) return nullable ? nullptr : "null pointer";
    if ((uintptr_t)p % 16) return "alignment: a base is not 16-byte aligned";
    if (ld % 8 != 0 || ld < width) return "stride: a 16-bit row stride is not a multiple of 8 or below the width";
    return nullptr;
}

inline const char *check_tail(const AnceLayerTail16Args *a, unsigned dtypes, bool backward) {
    if (!a) return "null pointer";
    if (a->H != 768 && a->H != 1024) return "width H not 768 or 1024";
    if (a->n_rows < 1) return "n_rows < 1";
    if (const char *why = check_dtype(a->dtype, dtypes)) return why;
    if (const char *why = check_matrix_t(a->dtype, a->x, a->ld_x, a->H)) return why;
    if (const char *why = check_matrix(a->res, a->ld_res, a->H)) return why;
    if (const char *why = check_vector(a->bias, true)) return why;
    if (const char *why = check_vector(a->gamma)) return why;
    if (!backward) {  // the backward touches neither y, y16 nor beta
        if (const char *why = check_matrix(a->y, a->ld_y, a->H)) return why;
        if (const char *why = check_matrix_t(a->dtype, a->y16, a->ld_y16, a->H, true)) return why;
        if (const char *why = check_vector(a->beta)) return why;
    }
    if (!(a->dropout_p >= 0.0f && a->dropout_p < 1.0f)) return "dropout_p outside [0, 1)";
    if (!(a->eps > 0.0f)) return "eps <= 0";
    return check_workspace(a->d_workspace, a->workspace_bytes, backward ? tail_ws_bytes(a->n_rows, a->H) : stats_bytes(a->n_rows));
}
// X's parameter block from checked arguments (the fp32 block has no y16 / dy16); g: the backward's, or null
template <class X>
typename X::Tail tail_params(const AnceLayerTail16Args *a, const AnceLayerTail16GradArgs *g, const uint64_t *d_stream) {
    typedef typename X::T T;
    typename X::Tail P = {};
    P.x = (const T *)a->x; P.res = a->res; P.bias = a->bias; P.gamma = a->gamma; P.beta = a->beta; P.y = a->y;
    P.ld_x = a->ld_x; P.ld_res = a->ld_res; P.ld_y = a->ld_y;
    if constexpr (X::HALF) { P.y16 = a->y16; P.ld_y16 = a->ld_y16; }
    if (g) {
        P.dy = g->dy; P.dx = (T *)g->dx; P.dres = g->dres;
        P.ld_dy = g->ld_dy; P.ld_dx = g->ld_dx; P.ld_dres = g->ld_dres;
        if constexpr (X::HALF) { P.dy16 = g->dy16; P.ld_dy16 = g->ld_dy16; }
    }
    P.n_rows = a->n_rows;
    P.mean = (float *)a->d_workspace;
    P.rstd = (float *)((char *)a->d_workspace + stats_bytes(a->n_rows) / 2);
    P.part = (float *)((char *)a->d_workspace + stats_bytes(a->n_rows));
    P.eps = a->eps;
    P.seed_lo = (uint32_t)a->seed; P.seed_hi = (uint32_t)(a->seed >> 32);
    P.off_lo = (uint32_t)a->offset; P.off_hi = (uint32_t)(a->offset >> 32);
    P.keep_thr = (uint32_t)((double)a->dropout_p * 4294967296.0);  // floor(p 2^32), p < 1
    P.keep_scale = 1.0f / (1.0f - a->dropout_p);
    P.d_stream = d_stream;
    return P;
}
inline bool drops(const AnceLayerTail16Args *a) { return a->training != 0 && a->dropout_p > 0.0f; }

inline const char *check_gelu(const AnceBiasGelu16Args *a, unsigned dtypes, bool backward) {
    if (!a) return "null pointer";
    if (a->N != 3072 && a->N != 4096) return "width N not 3072 or 4096";
    if (a->n_rows < 1) return "n_rows < 1";
    if (const char *why = check_dtype(a->dtype, dtypes)) return why;
    if (const char *why = check_matrix_t(a->dtype, a->x, a->ld_x, a->N)) return why;
    if (!backward) {  // the backward does not touch y
        if (const char *why = check_matrix_t(a->dtype, a->y, a->ld_y, a->N)) return why;
    }
    return check_vector(a->bias);
}
template <class X>
typename X::Gelu gelu_params(const AnceBiasGelu16Args *a, const AnceBiasGelu16GradArgs *g) {
    typedef typename X::T T;
    typename X::Gelu P = {};
    P.x = (const T *)a->x; P.bias = a->bias; P.y = (T *)a->y;
    P.ld_x = a->ld_x; P.ld_y = a->ld_y;
    if (g) {
        P.dy = (const T *)g->dy; P.dx = (T *)g->dx;
        P.ld_dy = g->ld_dy; P.ld_dx = g->ld_dx;
    }
    P.n_rows = a->n_rows;
    P.part = (float *)a->d_workspace;
    return P;
}

// launch(X{}) with the X of a checked dtype, among those of the family's mask
template <unsigned DTYPES, class Launch>
void by_dtype(int dtype, Launch launch) {
    if constexpr ((DTYPES & ONLY_F32) != 0) {
        if (dtype == ANCE_DTYPE_F32) return launch(F32{});
    }
    if constexpr ((DTYPES & ONLY_16) != 0) {
        if (dtype == ANCE_DTYPE_F16) launch(F16{});
        else launch(BF16{});
    }
}

// The call skeletons: everything is checked before anything is launched.
template <unsigned DTYPES>
int tail_forward(const char *fn, const AnceLayerTail16Args *args, const uint64_t *d_stream, void *stream) {
    if (!stream_aligned(d_stream)) return refuse(fn, "alignment: d_stream is not 16-byte aligned");
    if (const char *why = check_tail(args, DTYPES, false)) return refuse(fn, why);
    const dim3 grid((unsigned)n_part(args->n_rows));
    by_dtype<DTYPES>(args->dtype, [&](auto x) {
        typedef decltype(x) X;
        launch_tail_fwd<X>(args->H, drops(args), grid, (hipStream_t)stream, tail_params<X>(args, nullptr, d_stream));
    });
    return check_launch(fn);
}

template <unsigned DTYPES>
int tail_backward(const char *fn, const AnceLayerTail16Args *args, const AnceLayerTail16GradArgs *grads, const uint64_t *d_stream,
                  void *stream) {
    if (!stream_aligned(d_stream)) return refuse(fn, "alignment: d_stream is not 16-byte aligned");
    if (const char *why = check_tail(args, DTYPES, true)) return refuse(fn, why);
    if (!grads) return refuse(fn, "null pointer");
    // the fp32 family has dy alone; the 16-bit one takes dy, dy16 or both
    if (!grads->dy && !grads->dy16) return refuse(fn, args->dtype == ANCE_DTYPE_F32 ? "null pointer" : "null pointer: neither dy nor dy16");
    if (const char *why = check_matrix(grads->dy, grads->ld_dy, args->H, true)) return refuse(fn, why);
    if (const char *why = check_matrix_t(args->dtype, grads->dy16, grads->ld_dy16, args->H, true)) return refuse(fn, why);
    if (const char *why = check_matrix_t(args->dtype, grads->dx, grads->ld_dx, args->H, true)) return refuse(fn, why);
    if (const char *why = check_matrix(grads->dres, grads->ld_dres, args->H, true)) return refuse(fn, why);
    if (const char *why = check_vector(grads->dgamma, true)) return refuse(fn, why);
    if (const char *why = check_vector(grads->dbeta, true)) return refuse(fn, why);
    if (const char *why = check_vector(grads->dbias, true)) return refuse(fn, why);
    const dim3 grid((unsigned)n_part(args->n_rows));
    hipStream_t st = (hipStream_t)stream;
    float *dbias = args->bias ? grads->dbias : nullptr;  // no bias: no dbias
    by_dtype<DTYPES>(args->dtype, [&](auto x) {
        typedef decltype(x) X;
        const typename X::Tail P = tail_params<X>(args, grads, d_stream);
        launch_tail_bwd<X>(args->H, drops(args), grid, st, P);
        launch_tail_colsum(P.part, args->n_rows, args->H, grads->dgamma, grads->dbeta, dbias, st);
    });
    return check_launch(fn);
}

template <unsigned DTYPES>
int gelu_forward(const char *fn, const AnceBiasGelu16Args *args, void *stream) {
    if (const char *why = check_gelu(args, DTYPES, false)) return refuse(fn, why);
    const dim3 grid((unsigned)n_part(args->n_rows));
    by_dtype<DTYPES>(args->dtype, [&](auto x) {
        typedef decltype(x) X;
        launch_gelu_fwd<X>(args->N, grid, (hipStream_t)stream, gelu_params<X>(args, nullptr));
    });
    return check_launch(fn);
}

template <unsigned DTYPES>
int gelu_backward(const char *fn, const AnceBiasGelu16Args *args, const AnceBiasGelu16GradArgs *grads, void *stream) {
    if (const char *why = check_gelu(args, DTYPES, true)) return refuse(fn, why);
    if (const char *why = check_workspace(args->d_workspace, args->workspace_bytes, gelu_ws_bytes(args->n_rows, args->N))) return refuse(fn, why);
    if (!grads) return refuse(fn, "null pointer");
    if (const char *why = check_matrix_t(args->dtype, grads->dy, grads->ld_dy, args->N)) return refuse(fn, why);
    if (const char *why = check_matrix_t(args->dtype, grads->dx, grads->ld_dx, args->N, true)) return refuse(fn, why);
    if (const char *why = check_vector(grads->dbias, true)) return refuse(fn, why);
    const dim3 grid((unsigned)n_part(args->n_rows));
    hipStream_t st = (hipStream_t)stream;
    by_dtype<DTYPES>(args->dtype, [&](auto x) {
        typedef decltype(x) X;
        const typename X::Gelu P = gelu_params<X>(args, grads);
        launch_gelu_bwd<X>(args->N, grid, st, P);
        launch_gelu_colsum(P.part, args->n_rows, args->N, grads->dbias, st);
    });
    return check_launch(fn);
}

// the workspace queries of both families: 0 for what is not supported
inline size_t tail_ws_query(int64_t n_rows, int H) { return rows_ok(n_rows) && (H == 768 || H == 1024) ? tail_ws_bytes(n_rows, H) : 0; }
inline size_t gelu_ws_query(int64_t n_rows, int N) { return rows_ok(n_rows) && (N == 3072 || N == 4096) ? gelu_ws_bytes(n_rows, N) : 0; }

}  // namespace
}  // namespace ance
