// The row-wise seams of a BertLayer with 16-bit matmul-side I/O and an fp32 residual stream (include/ance_amd.h: ance_layer_tail16_*
// and ance_bias_gelu16_*): the 16-bit counterpart of layer_tail.hip, as attention_train_half.hip is of attention_train.hip.
//   tail   x is T (fp16 or bf16), res / y / bias / gamma / beta fp32;  u = float(x) + bias, then layer_tail.hip's arithmetic in fp32,
//          expression for expression: on an x that holds T values y, dres, dgamma, dbeta, dbias are the fp32 tail's bits on float(x).
//          y16 (optional) is y's registers rounded once.  backward: g = dy + float(dy16) (each optional, one given) in registers;
//          dx is T, rounded once, overflow to +-inf; dbias sums the unrounded dx.
//   gelu   x, y, dy, dx are T, bias / dbias fp32;  u = float(x) + bias, the erf form in fp32, one rounding at each store.
// The layout is the fp32 kernels' own: one wave owns a row, lane l holds columns 4 (64 i + l) .. + 3, i < width / 256 -- an 8-byte
// access of a T row (512 B contiguous per wave) next to a 16-byte access of an fp32 row.  768 / 64 lanes = 12 halves = 24 bytes, so
// 16 bytes per lane of a T row do not divide the tail's widths; and with this layout the Philox call per four columns, the wave
// reductions, write_partial and colsum_tree_kernel (row_kernels.h) are used as they are.  The GELU keeps the same layout so that its
// dbias goes through the same partial rows.  Rounding is the compiler's float -> T conversion: to nearest even, +-inf on overflow.
// The kernels are layer_tail_kernels.h's, instantiated here with X = F16 / BF16 (layer_tail.hip: X = F32): one text for both
// precisions.  This file holds the argument checks and the entry points.
#include "layer_tail_kernels.h"

namespace ance {
namespace {

// check_matrix for a T matrix: 16-byte pieces of 16-bit elements, so a row stride is a multiple of 8
const char *check_matrix16(const void *p, int ld, int width, bool nullable = false) {
    if (!p) return nullable ? nullptr : "null pointer";
    if ((uintptr_t)p % 16) return "alignment: a base is not 16-byte aligned";
    if (ld % 8 != 0 || ld < width) return "stride: a 16-bit row stride is not a multiple of 8 or below the width";
    return nullptr;
}
const char *check_dtype(int dtype) { return dtype == ANCE_DTYPE_F16 || dtype == ANCE_DTYPE_BF16 ? nullptr : "dtype neither ANCE_DTYPE_F16 nor ANCE_DTYPE_BF16"; }

const char *check_tail(const AnceLayerTail16Args *a, bool backward) {
    if (!a) return "null pointer";
    if (a->H != 768 && a->H != 1024) return "width H not 768 or 1024";
    if (a->n_rows < 1) return "n_rows < 1";
    if (const char *why = check_dtype(a->dtype)) return why;
    if (const char *why = check_matrix16(a->x, a->ld_x, a->H)) return why;
    if (const char *why = check_matrix(a->res, a->ld_res, a->H)) return why;
    if (const char *why = check_vector(a->bias, true)) return why;
    if (const char *why = check_vector(a->gamma)) return why;
    if (!backward) {  // the backward touches neither y, y16 nor beta
        if (const char *why = check_matrix(a->y, a->ld_y, a->H)) return why;
        if (const char *why = check_matrix16(a->y16, a->ld_y16, a->H, true)) return why;
        if (const char *why = check_vector(a->beta)) return why;
    }
    if (!(a->dropout_p >= 0.0f && a->dropout_p < 1.0f)) return "dropout_p outside [0, 1)";
    if (!(a->eps > 0.0f)) return "eps <= 0";
    return check_workspace(a->d_workspace, a->workspace_bytes, backward ? tail_ws_bytes(a->n_rows, a->H) : stats_bytes(a->n_rows));
}
TailParams16 tail_params(const AnceLayerTail16Args *a, const uint64_t *d_stream) {
    TailParams16 P = {};
    P.x = a->x; P.res = a->res; P.bias = a->bias; P.gamma = a->gamma; P.beta = a->beta; P.y = a->y; P.y16 = a->y16;
    P.ld_x = a->ld_x; P.ld_res = a->ld_res; P.ld_y = a->ld_y; P.ld_y16 = a->ld_y16;
    fill_tail_common(P, a);
    P.d_stream = d_stream;
    return P;
}
bool drops(const AnceLayerTail16Args *a) { return a->training != 0 && a->dropout_p > 0.0f; }

const char *check_gelu(const AnceBiasGelu16Args *a, bool backward) {
    if (!a) return "null pointer";
    if (a->N != 3072 && a->N != 4096) return "width N not 3072 or 4096";
    if (a->n_rows < 1) return "n_rows < 1";
    if (const char *why = check_dtype(a->dtype)) return why;
    if (const char *why = check_matrix16(a->x, a->ld_x, a->N)) return why;
    if (!backward) {  // the backward does not touch y
        if (const char *why = check_matrix16(a->y, a->ld_y, a->N)) return why;
    }
    return check_vector(a->bias);
}
GeluParams16 gelu_params(const AnceBiasGelu16Args *a) {
    GeluParams16 P = {};
    P.x = a->x; P.bias = a->bias; P.y = a->y;
    P.ld_x = a->ld_x; P.ld_y = a->ld_y;
    P.n_rows = a->n_rows;
    P.part = (float *)a->d_workspace;
    return P;
}

}  // namespace
}  // namespace ance

extern "C" size_t ance_layer_tail16_workspace_bytes(int64_t n_rows, int H) {
    using namespace ance;
    return rows_ok(n_rows) && (H == 768 || H == 1024) ? tail_ws_bytes(n_rows, H) : 0;
}

extern "C" size_t ance_bias_gelu16_workspace_bytes(int64_t n_rows, int N) {
    using namespace ance;
    return rows_ok(n_rows) && (N == 3072 || N == 4096) ? gelu_ws_bytes(n_rows, N) : 0;
}

static int ance_layer_tail16_forward_impl(const char *fn, const AnceLayerTail16Args *args, const uint64_t *d_stream, void *stream) {
    using namespace ance;
    if (!stream_aligned(d_stream)) return refuse(fn, "alignment: d_stream is not 16-byte aligned");
    if (const char *why = check_tail(args, false)) return refuse(fn, why);
    const TailParams16 P = tail_params(args, d_stream);
    const dim3 grid((unsigned)n_part(args->n_rows));
    hipStream_t st = (hipStream_t)stream;
    if (args->dtype == ANCE_DTYPE_F16) launch_tail_fwd<F16>(args->H, drops(args), grid, st, P);
    else launch_tail_fwd<BF16>(args->H, drops(args), grid, st, P);
    return check_launch(fn);
}

static int ance_layer_tail16_backward_impl(const char *fn, const AnceLayerTail16Args *args, const AnceLayerTail16GradArgs *grads,
                                           const uint64_t *d_stream, void *stream) {
    using namespace ance;
    if (!stream_aligned(d_stream)) return refuse(fn, "alignment: d_stream is not 16-byte aligned");
    if (const char *why = check_tail(args, true)) return refuse(fn, why);
    if (!grads) return refuse(fn, "null pointer");
    if (!grads->dy && !grads->dy16) return refuse(fn, "null pointer: neither dy nor dy16");
    if (const char *why = check_matrix(grads->dy, grads->ld_dy, args->H, true)) return refuse(fn, why);
    if (const char *why = check_matrix16(grads->dy16, grads->ld_dy16, args->H, true)) return refuse(fn, why);
    if (const char *why = check_matrix16(grads->dx, grads->ld_dx, args->H, true)) return refuse(fn, why);
    if (const char *why = check_matrix(grads->dres, grads->ld_dres, args->H, true)) return refuse(fn, why);
    if (const char *why = check_vector(grads->dgamma, true)) return refuse(fn, why);
    if (const char *why = check_vector(grads->dbeta, true)) return refuse(fn, why);
    if (const char *why = check_vector(grads->dbias, true)) return refuse(fn, why);
    TailParams16 P = tail_params(args, d_stream);
    P.dy = grads->dy; P.dy16 = grads->dy16; P.dx = grads->dx; P.dres = grads->dres;
    P.ld_dy = grads->ld_dy; P.ld_dy16 = grads->ld_dy16; P.ld_dx = grads->ld_dx; P.ld_dres = grads->ld_dres;
    const dim3 grid((unsigned)n_part(args->n_rows));
    hipStream_t st = (hipStream_t)stream;
    if (args->dtype == ANCE_DTYPE_F16) launch_tail_bwd<F16>(args->H, drops(args), grid, st, P);
    else launch_tail_bwd<BF16>(args->H, drops(args), grid, st, P);
    float *dbias = args->bias ? grads->dbias : nullptr;  // no bias: no dbias
    launch_tail_colsum(P.part, args->n_rows, args->H, grads->dgamma, grads->dbeta, dbias, st);
    return check_launch(fn);
}

extern "C" int ance_bias_gelu16_forward(const AnceBiasGelu16Args *args, void *stream) {
    using namespace ance;
    const char *fn = "ance_bias_gelu16_forward";
    if (const char *why = check_gelu(args, false)) return refuse(fn, why);
    const GeluParams16 P = gelu_params(args);
    const dim3 grid((unsigned)n_part(args->n_rows));
    hipStream_t st = (hipStream_t)stream;
    if (args->dtype == ANCE_DTYPE_F16) launch_gelu_fwd<F16>(args->N, grid, st, P);
    else launch_gelu_fwd<BF16>(args->N, grid, st, P);
    return check_launch(fn);
}

extern "C" int ance_bias_gelu16_backward(const AnceBiasGelu16Args *args, const AnceBiasGelu16GradArgs *grads, void *stream) {
    using namespace ance;
    const char *fn = "ance_bias_gelu16_backward";
    if (const char *why = check_gelu(args, true)) return refuse(fn, why);
    if (const char *why = check_workspace(args->d_workspace, args->workspace_bytes, gelu_ws_bytes(args->n_rows, args->N))) return refuse(fn, why);
    if (!grads) return refuse(fn, "null pointer");
    if (const char *why = check_matrix16(grads->dy, grads->ld_dy, args->N)) return refuse(fn, why);
    if (const char *why = check_matrix16(grads->dx, grads->ld_dx, args->N, true)) return refuse(fn, why);
    if (const char *why = check_vector(grads->dbias, true)) return refuse(fn, why);
    GeluParams16 P = gelu_params(args);
    P.dy = grads->dy; P.dx = grads->dx;
    P.ld_dy = grads->ld_dy; P.ld_dx = grads->ld_dx;
    const dim3 grid((unsigned)n_part(args->n_rows));
    hipStream_t st = (hipStream_t)stream;
    if (args->dtype == ANCE_DTYPE_F16) launch_gelu_bwd<F16>(args->N, grid, st, P);
    else launch_gelu_bwd<BF16>(args->N, grid, st, P);
    launch_gelu_colsum(P.part, args->n_rows, args->N, grads->dbias, st);
    return check_launch(fn);
}

// The entry points: each with its sibling that takes the device dropout stream (include/ance_amd.h); the plain one passes none.
extern "C" int ance_layer_tail16_forward(const AnceLayerTail16Args *args, void *stream) {
    return ance_layer_tail16_forward_impl("ance_layer_tail16_forward", args, nullptr, stream);
}
extern "C" int ance_layer_tail16_forward_dstream(const AnceLayerTail16Args *args, const uint64_t *d_stream, void *stream) {
    return ance_layer_tail16_forward_impl("ance_layer_tail16_forward_dstream", args, d_stream, stream);
}
extern "C" int ance_layer_tail16_backward(const AnceLayerTail16Args *args, const AnceLayerTail16GradArgs *grads, void *stream) {
    return ance_layer_tail16_backward_impl("ance_layer_tail16_backward", args, grads, nullptr, stream);
}
extern "C" int ance_layer_tail16_backward_dstream(const AnceLayerTail16Args *args, const AnceLayerTail16GradArgs *grads,
                                                  const uint64_t *d_stream, void *stream) {
    return ance_layer_tail16_backward_impl("ance_layer_tail16_backward_dstream", args, grads, d_stream, stream);
}
