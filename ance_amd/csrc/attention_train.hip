// The trainers' self-attention core in fp32 (include/ance_amd.h: ance_attention_forward / ance_attention_backward): the kernels of
// attention_train_kernels.h with X = F32 -- the mathematics, the layout and the fp32 policy are stated there -- behind the front end
// of attention_common.h.  Here: the fp32 argument structs in their internal form, and the entry points.
#include "attention_train_kernels.h"

namespace ance {
namespace {

// the fp32 structs as the internal ones (the same fields; reserved becomes the dtype); null stays null
const AnceAttn16Args *internal(const AnceAttnTrainArgs *a, AnceAttn16Args *out) {
    if (!a) return nullptr;
    *out = AnceAttn16Args{a->q, a->k, a->v, a->ctx, a->ld_q, a->ld_k, a->ld_v, a->ld_ctx, a->d_seq_first, a->d_seq_len, a->n_seq,
                          a->max_seq_len, a->n_rows, a->n_heads, a->seq_rows, ANCE_DTYPE_F32, a->dropout_p, a->training, a->seed,
                          a->offset, a->d_workspace, a->workspace_bytes};
    return out;
}
const AnceAttn16GradArgs *internal(const AnceAttnGradArgs *g, AnceAttn16GradArgs *out) {
    if (!g) return nullptr;
    *out = AnceAttn16GradArgs{g->dctx, g->dq, g->dk, g->dv, g->ld_dctx, g->ld_dq, g->ld_dk, g->ld_dv};
    return out;
}

int forward(const char *fn, const AnceAttnTrainArgs *args, const uint64_t *d_stream, void *stream) {
    AnceAttn16Args a;
    return core_call(fn, 1u << ANCE_DTYPE_F32, internal(args, &a), false, nullptr, d_stream,
                     [&](const AttnParams &P) { launch_forward<F32>(&a, P, (hipStream_t)stream); });
}
int backward(const char *fn, const AnceAttnTrainArgs *args, const AnceAttnGradArgs *grads, const uint64_t *d_stream, void *stream) {
    AnceAttn16Args a;
    AnceAttn16GradArgs g;
    return core_call(fn, 1u << ANCE_DTYPE_F32, internal(args, &a), true, internal(grads, &g), d_stream,
                     [&](const AttnParams &P) { launch_backward<F32>(&a, P, (hipStream_t)stream); });
}

}  // namespace
}  // namespace ance

extern "C" size_t ance_attention_workspace_bytes(int64_t n_rows, int n_heads) { return ance::core_workspace_query(n_rows, n_heads); }

// The entry points: each with its sibling that takes the device dropout stream (include/ance_amd.h); the plain one passes none.
extern "C" int ance_attention_forward(const AnceAttnTrainArgs *args, void *stream) {
    return ance::forward("ance_attention_forward", args, nullptr, stream);
}
extern "C" int ance_attention_forward_dstream(const AnceAttnTrainArgs *args, const uint64_t *d_stream, void *stream) {
    return ance::forward("ance_attention_forward_dstream", args, d_stream, stream);
}
extern "C" int ance_attention_backward(const AnceAttnTrainArgs *args, const AnceAttnGradArgs *grads, void *stream) {
    return ance::backward("ance_attention_backward", args, grads, nullptr, stream);
}
extern "C" int ance_attention_backward_dstream(const AnceAttnTrainArgs *args, const AnceAttnGradArgs *grads, const uint64_t *d_stream,
                                               void *stream) {
    return ance::backward("ance_attention_backward_dstream", args, grads, d_stream, stream);
}
