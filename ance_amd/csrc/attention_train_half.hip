// The trainers' self-attention core in 16-bit I/O (include/ance_amd.h: ance_attention16_forward / ance_attention16_backward): the
// kernels of attention_train_kernels.h with X = F16 / BF16 -- q, k, v, ctx, dctx, dq, dk, dv as fp16 or bf16 rows, every product on
// the 16-bit matrix cores; the arithmetic contract and the operand maps are stated there with the 16-bit policy -- behind the front
// end of attention_common.h.  Here: the choice of the instantiation, and the entry points.
#include "attention_train_kernels.h"

namespace ance {
namespace {

constexpr unsigned HALF_DTYPES = 1u << ANCE_DTYPE_F16 | 1u << ANCE_DTYPE_BF16;

int forward(const char *fn, const AnceAttn16Args *args, const uint64_t *d_stream, void *stream) {
    return core_call(fn, HALF_DTYPES, args, false, nullptr, d_stream, [&](const AttnParams &P) {
        if (args->dtype == ANCE_DTYPE_F16) launch_forward<F16>(args, P, (hipStream_t)stream);
        else launch_forward<BF16>(args, P, (hipStream_t)stream);
    });
}
int backward(const char *fn, const AnceAttn16Args *args, const AnceAttn16GradArgs *grads, const uint64_t *d_stream, void *stream) {
    return core_call(fn, HALF_DTYPES, args, true, grads, d_stream, [&](const AttnParams &P) {
        if (args->dtype == ANCE_DTYPE_F16) launch_backward<F16>(args, P, (hipStream_t)stream);
        else launch_backward<BF16>(args, P, (hipStream_t)stream);
    });
}

}  // namespace
}  // namespace ance

extern "C" size_t ance_attention16_workspace_bytes(int64_t n_rows, int n_heads) { return ance::core_workspace_query(n_rows, n_heads); }

// The entry points: each with its sibling that takes the device dropout stream (include/ance_amd.h); the plain one passes none.
extern "C" int ance_attention16_forward(const AnceAttn16Args *args, void *stream) {
    return ance::forward("ance_attention16_forward", args, nullptr, stream);
}
extern "C" int ance_attention16_forward_dstream(const AnceAttn16Args *args, const uint64_t *d_stream, void *stream) {
    return ance::forward("ance_attention16_forward_dstream", args, d_stream, stream);
}
extern "C" int ance_attention16_backward(const AnceAttn16Args *args, const AnceAttn16GradArgs *grads, void *stream) {
    return ance::backward("ance_attention16_backward", args, grads, nullptr, stream);
}
extern "C" int ance_attention16_backward_dstream(const AnceAttn16Args *args, const AnceAttn16GradArgs *grads, const uint64_t *d_stream,
                                                 void *stream) {
    return ance::backward("ance_attention16_backward_dstream", args, grads, d_stream, stream);
}
