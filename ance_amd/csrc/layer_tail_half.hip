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
// precisions, behind the one front end of layer_tail_common.h, whose internal form these structs are.  Here: the entry points.
#include "layer_tail_common.h"

using ance::ONLY_16;

extern "C" size_t ance_layer_tail16_workspace_bytes(int64_t n_rows, int H) { return ance::tail_ws_query(n_rows, H); }
extern "C" size_t ance_bias_gelu16_workspace_bytes(int64_t n_rows, int N) { return ance::gelu_ws_query(n_rows, N); }

extern "C" int ance_bias_gelu16_forward(const AnceBiasGelu16Args *args, void *stream) {
    return ance::gelu_forward<ONLY_16>("ance_bias_gelu16_forward", args, stream);
}
extern "C" int ance_bias_gelu16_backward(const AnceBiasGelu16Args *args, const AnceBiasGelu16GradArgs *grads, void *stream) {
    return ance::gelu_backward<ONLY_16>("ance_bias_gelu16_backward", args, grads, stream);
}

// The tail's entry points: each with its sibling that takes the device dropout stream (include/ance_amd.h); the plain one passes none.
extern "C" int ance_layer_tail16_forward(const AnceLayerTail16Args *args, void *stream) {
    return ance::tail_forward<ONLY_16>("ance_layer_tail16_forward", args, nullptr, stream);
}
extern "C" int ance_layer_tail16_forward_dstream(const AnceLayerTail16Args *args, const uint64_t *d_stream, void *stream) {
    return ance::tail_forward<ONLY_16>("ance_layer_tail16_forward_dstream", args, d_stream, stream);
}
extern "C" int ance_layer_tail16_backward(const AnceLayerTail16Args *args, const AnceLayerTail16GradArgs *grads, void *stream) {
    return ance::tail_backward<ONLY_16>("ance_layer_tail16_backward", args, grads, nullptr, stream);
}
extern "C" int ance_layer_tail16_backward_dstream(const AnceLayerTail16Args *args, const AnceLayerTail16GradArgs *grads,
                                                  const uint64_t *d_stream, void *stream) {
    return ance::tail_backward<ONLY_16>("ance_layer_tail16_backward_dstream", args, grads, d_stream, stream);
}
