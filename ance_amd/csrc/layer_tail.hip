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
// The kernels themselves are layer_tail_kernels.h's, instantiated here with fp32 rows (X = F32) and in layer_tail_half.hip with
// 16-bit ones.
#include "layer_tail_kernels.h"

namespace ance {
namespace {

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
TailParams tail_params(const AnceLayerTailArgs *a, const uint64_t *d_stream) {
    TailParams P = {};
    P.x = a->x; P.res = a->res; P.bias = a->bias; P.gamma = a->gamma; P.beta = a->beta; P.y = a->y;
    P.ld_x = a->ld_x; P.ld_res = a->ld_res; P.ld_y = a->ld_y;
    fill_tail_common(P, a);
    P.d_stream = d_stream;
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

extern "C" int ance_layer_tail_rows_per_workgroup(void) {
    return ance::LT_ROWS;
}

extern "C" size_t ance_layer_tail_workspace_bytes(int64_t n_rows, int H) {
    using namespace ance;
    return rows_ok(n_rows) && (H == 768 || H == 1024) ? tail_ws_bytes(n_rows, H) : 0;
}

extern "C" size_t ance_bias_gelu_workspace_bytes(int64_t n_rows, int N) {
    using namespace ance;
    return rows_ok(n_rows) && (N == 3072 || N == 4096) ? gelu_ws_bytes(n_rows, N) : 0;
}

static int ance_layer_tail_forward_impl(const char *fn, const AnceLayerTailArgs *args, const uint64_t *d_stream, void *stream) {
    using namespace ance;
    if (!stream_aligned(d_stream)) return refuse(fn, "alignment: d_stream is not 16-byte aligned");
    if (const char *why = check_tail(args, false)) return refuse(fn, why);
    const TailParams P = tail_params(args, d_stream);
    launch_tail_fwd<F32>(args->H, drops(args), dim3((unsigned)n_part(args->n_rows)), (hipStream_t)stream, P);
    return check_launch(fn);
}

static int ance_layer_tail_backward_impl(const char *fn, const AnceLayerTailArgs *args, const AnceLayerTailGradArgs *grads,
                                         const uint64_t *d_stream, void *stream) {
    using namespace ance;
    if (!stream_aligned(d_stream)) return refuse(fn, "alignment: d_stream is not 16-byte aligned");
    if (const char *why = check_tail(args, true)) return refuse(fn, why);
    if (!grads) return refuse(fn, "null pointer");
    if (const char *why = check_matrix(grads->dy, grads->ld_dy, args->H)) return refuse(fn, why);
    if (const char *why = check_matrix(grads->dx, grads->ld_dx, args->H, true)) return refuse(fn, why);
    if (const char *why = check_matrix(grads->dres, grads->ld_dres, args->H, true)) return refuse(fn, why);
    if (const char *why = check_vector(grads->dgamma, true)) return refuse(fn, why);
    if (const char *why = check_vector(grads->dbeta, true)) return refuse(fn, why);
    if (const char *why = check_vector(grads->dbias, true)) return refuse(fn, why);
    TailParams P = tail_params(args, d_stream);
    P.dy = grads->dy; P.dx = grads->dx; P.dres = grads->dres;
    P.ld_dy = grads->ld_dy; P.ld_dx = grads->ld_dx; P.ld_dres = grads->ld_dres;
    hipStream_t st = (hipStream_t)stream;
    launch_tail_bwd<F32>(args->H, drops(args), dim3((unsigned)n_part(args->n_rows)), st, P);
    float *dbias = args->bias ? grads->dbias : nullptr;  // no bias: no dbias
    launch_tail_colsum(P.part, args->n_rows, args->H, grads->dgamma, grads->dbeta, dbias, st);
    return check_launch(fn);
}

extern "C" int ance_bias_gelu_forward(const AnceBiasGeluArgs *args, void *stream) {
    using namespace ance;
    const char *fn = "ance_bias_gelu_forward";
    if (const char *why = check_gelu(args, false)) return refuse(fn, why);
    const GeluParams P = gelu_params(args);
    launch_gelu_fwd<F32>(args->N, dim3((unsigned)n_part(args->n_rows)), (hipStream_t)stream, P);
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
    hipStream_t st = (hipStream_t)stream;
    launch_gelu_bwd<F32>(args->N, dim3((unsigned)n_part(args->n_rows)), st, P);
    launch_gelu_colsum(P.part, args->n_rows, args->N, grads->dbias, st);
    return check_launch(fn);
}

// The entry points: each with its sibling that takes the device dropout stream (include/ance_amd.h); the plain one passes none.
extern "C" int ance_layer_tail_forward(const AnceLayerTailArgs *args, void *stream) {
    return ance_layer_tail_forward_impl("ance_layer_tail_forward", args, nullptr, stream);
}
extern "C" int ance_layer_tail_forward_dstream(const AnceLayerTailArgs *args, const uint64_t *d_stream, void *stream) {
    return ance_layer_tail_forward_impl("ance_layer_tail_forward_dstream", args, d_stream, stream);
}
extern "C" int ance_layer_tail_backward(const AnceLayerTailArgs *args, const AnceLayerTailGradArgs *grads, void *stream) {
    return ance_layer_tail_backward_impl("ance_layer_tail_backward", args, grads, nullptr, stream);
}
extern "C" int ance_layer_tail_backward_dstream(const AnceLayerTailArgs *args, const AnceLayerTailGradArgs *grads,
                                                const uint64_t *d_stream, void *stream) {
    return ance_layer_tail_backward_impl("ance_layer_tail_backward_dstream", args, grads, d_stream, stream);
}
