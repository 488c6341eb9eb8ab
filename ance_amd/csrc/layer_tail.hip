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
// The row reductions, the partial rows, the column-sum tree and the fp32 argument checks are row_kernels.h's, shared with
// embed_train.hip.  The kernels are layer_tail_kernels.h's with fp32 rows (X = F32), behind the front end of layer_tail_common.h.
// Here: the fp32 argument structs in their internal form, and the entry points.
#include "layer_tail_common.h"

namespace ance {
namespace {

// the fp32 structs as the internal ones (dtype ANCE_DTYPE_F32, no y16 / dy16); null stays null
const AnceLayerTail16Args *internal(const AnceLayerTailArgs *a, AnceLayerTail16Args *out) {
    if (!a) return nullptr;
    *out = AnceLayerTail16Args{a->x, a->res, a->bias, a->gamma, a->beta, a->y, nullptr, a->ld_x, a->ld_res, a->ld_y, 0, a->H, a->n_rows,
                               ANCE_DTYPE_F32, a->eps, a->dropout_p, a->training, a->seed, a->offset, a->d_workspace, a->workspace_bytes};
    return out;
}
const AnceLayerTail16GradArgs *internal(const AnceLayerTailGradArgs *g, AnceLayerTail16GradArgs *out) {
    if (!g) return nullptr;
    *out = AnceLayerTail16GradArgs{g->dy, nullptr, g->dx, g->dres, g->dgamma, g->dbeta, g->dbias, g->ld_dy, 0, g->ld_dx, g->ld_dres};
    return out;
}
const AnceBiasGelu16Args *internal(const AnceBiasGeluArgs *a, AnceBiasGelu16Args *out) {
    if (!a) return nullptr;
    *out = AnceBiasGelu16Args{a->x, a->bias, a->y, a->ld_x, a->ld_y, a->N, a->n_rows, ANCE_DTYPE_F32, 0, a->d_workspace, a->workspace_bytes};
    return out;
}
const AnceBiasGelu16GradArgs *internal(const AnceBiasGeluGradArgs *g, AnceBiasGelu16GradArgs *out) {
    if (!g) return nullptr;
    *out = AnceBiasGelu16GradArgs{g->dy, g->dx, g->dbias, g->ld_dy, g->ld_dx};
    return out;
}

int forward(const char *fn, const AnceLayerTailArgs *args, const uint64_t *d_stream, void *stream) {
    AnceLayerTail16Args a;
    return tail_forward<ONLY_F32>(fn, internal(args, &a), d_stream, stream);
}
int backward(const char *fn, const AnceLayerTailArgs *args, const AnceLayerTailGradArgs *grads, const uint64_t *d_stream, void *stream) {
    AnceLayerTail16Args a;
    AnceLayerTail16GradArgs g;
    return tail_backward<ONLY_F32>(fn, internal(args, &a), internal(grads, &g), d_stream, stream);
}

}  // namespace
}  // namespace ance

extern "C" int ance_layer_tail_rows_per_workgroup(void) { return ance::LT_ROWS; }
extern "C" size_t ance_layer_tail_workspace_bytes(int64_t n_rows, int H) { return ance::tail_ws_query(n_rows, H); }
extern "C" size_t ance_bias_gelu_workspace_bytes(int64_t n_rows, int N) { return ance::gelu_ws_query(n_rows, N); }

extern "C" int ance_bias_gelu_forward(const AnceBiasGeluArgs *args, void *stream) {
    AnceBiasGelu16Args a;
    return ance::gelu_forward<ance::ONLY_F32>("ance_bias_gelu_forward", ance::internal(args, &a), stream);
}
extern "C" int ance_bias_gelu_backward(const AnceBiasGeluArgs *args, const AnceBiasGeluGradArgs *grads, void *stream) {
    AnceBiasGelu16Args a;
    AnceBiasGelu16GradArgs g;
    return ance::gelu_backward<ance::ONLY_F32>("ance_bias_gelu_backward", ance::internal(args, &a), ance::internal(grads, &g), stream);
}

// The tail's entry points: each with its sibling that takes the device dropout stream (include/ance_amd.h); the plain one passes none.
extern "C" int ance_layer_tail_forward(const AnceLayerTailArgs *args, void *stream) {
    return ance::forward("ance_layer_tail_forward", args, nullptr, stream);
}
extern "C" int ance_layer_tail_forward_dstream(const AnceLayerTailArgs *args, const uint64_t *d_stream, void *stream) {
    return ance::forward("ance_layer_tail_forward_dstream", args, d_stream, stream);
}
extern "C" int ance_layer_tail_backward(const AnceLayerTailArgs *args, const AnceLayerTailGradArgs *grads, void *stream) {
    return ance::backward("ance_layer_tail_backward", args, grads, nullptr, stream);
}
extern "C" int ance_layer_tail_backward_dstream(const AnceLayerTailArgs *args, const AnceLayerTailGradArgs *grads,
                                                const uint64_t *d_stream, void *stream) {
    return ance::backward("ance_layer_tail_backward_dstream", args, grads, d_stream, stream);
}
