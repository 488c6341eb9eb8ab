// What the trainers' three attention files share (attention_train.hip, attention_train_half.hip, attention_row0.hip): the device's
// view of a sequence descriptor, and the host front end -- one argument check, one parameter fill and one call skeleton over
// AnceAttn16Args / AnceAttn16GradArgs, the internal form of every entry point (the fp32 core converts its own structs once).
#pragma once
#include "common.h"
#include "philox.h"

namespace ance {
namespace {

// first row and clamped length of sequence s: never a row outside [0, n_rows), whatever the descriptors say
template <class Params>
__device__ __forceinline__ int seq_bounds(const Params &P, int s, int *first) {
    const int f = P.seq_first[s];
    int len = P.seq_len[s];
    *first = f;
    if (f < 0 || f >= P.n_rows || len < 0) return 0;
    if (len > P.max_seq_len) len = P.max_seq_len;
    if (len > P.n_rows - f) len = P.n_rows - f;
    return len;
}

// the shapes a workspace query answers for: n rows (the full core) or sequences (the first-row core), at most n_max
inline bool shape_ok(int64_t n, int64_t n_max, int n_heads) { return n >= 1 && n <= n_max && (n_heads == 12 || n_heads == 16); }
inline int piece_elems(int dtype) { return dtype == ANCE_DTYPE_F32 ? 4 : 8; }  // elements of a 16-byte piece of a row

const char *check_matrix(const void *p, int ld, int n_heads, int piece) {
    if (!p) return "null pointer";
    if ((uintptr_t)p % 16) return "alignment: a base is not 16-byte aligned";
    if (ld % piece != 0 || ld < 64 * n_heads) return "stride: not a multiple of a 16-byte piece or below 64 * n_heads";
    return nullptr;
}

// What an entry point accepts beyond the common rules: its dtypes (bit 1 << ANCE_DTYPE_*) and the workspace its shape needs
struct AttnRules {
    unsigned dtypes;
    const char *dtype_why;
    size_t ws_bytes;
};

const char *check_args(const AnceAttn16Args *a, const AttnRules &rules) {
    if (!a) return "null pointer";
    if (a->dtype < 0 || a->dtype > 31 || !(rules.dtypes >> a->dtype & 1u)) return rules.dtype_why;
    if (a->n_heads != 12 && a->n_heads != 16) return "n_heads not 12 or 16";
    if (a->max_seq_len < 1 || a->max_seq_len > 512) return "max_seq_len outside 1 .. 512";
    if (a->n_seq < 1 || a->n_seq > 65535) return "n_seq outside 1 .. 65535";
    if (a->n_rows < 1) return "n_rows < 1";
    if (a->seq_rows < 0 || a->seq_rows > a->max_seq_len) return "seq_rows outside 0 .. max_seq_len";
    if (!a->d_seq_first || !a->d_seq_len) return "null pointer";
    const int piece = piece_elems(a->dtype);
    if (const char *why = check_matrix(a->q, a->ld_q, a->n_heads, piece)) return why;
    if (const char *why = check_matrix(a->k, a->ld_k, a->n_heads, piece)) return why;
    if (const char *why = check_matrix(a->v, a->ld_v, a->n_heads, piece)) return why;
    if (const char *why = check_matrix(a->ctx, a->ld_ctx, a->n_heads, piece)) return why;
    if (!(a->dropout_p >= 0.0f && a->dropout_p < 1.0f)) return "dropout_p outside [0, 1)";
    if (!a->d_workspace || (uintptr_t)a->d_workspace % 16) return "null or unaligned workspace";
    if (a->workspace_bytes < rules.ws_bytes) return "workspace too small";
    return nullptr;
}

bool drops(const AnceAttn16Args *a) { return a->training != 0 && a->dropout_p > 0.0f; }

// The fields every parameter block has (AttnParams, Row0Params), from checked arguments; g: the backward's, or null
template <class Params>
Params params(const AnceAttn16Args *a, const AnceAttn16GradArgs *g, const uint64_t *d_stream) {
    Params P = {};
    P.q = a->q; P.k = a->k; P.v = a->v; P.ctx = a->ctx;
    P.ld_q = a->ld_q; P.ld_k = a->ld_k; P.ld_v = a->ld_v; P.ld_ctx = a->ld_ctx;
    if (g) {
        P.dctx = g->dctx; P.dq = g->dq; P.dk = g->dk; P.dv = g->dv;
        P.ld_dctx = g->ld_dctx; P.ld_dq = g->ld_dq; P.ld_dk = g->ld_dk; P.ld_dv = g->ld_dv;
    }
    P.seq_first = a->d_seq_first; P.seq_len = a->d_seq_len;
    P.max_seq_len = a->max_seq_len; P.n_rows = a->n_rows; P.n_heads = a->n_heads; P.seq_rows = a->seq_rows;
    P.seed_lo = (uint32_t)a->seed; P.seed_hi = (uint32_t)(a->seed >> 32);
    P.off_lo = (uint32_t)a->offset; P.off_hi = (uint32_t)(a->offset >> 32);
    P.d_stream = d_stream;  // given: seed and base come from the device, a->offset is added to the base
    P.keep_thr = (uint32_t)((double)a->dropout_p * 4294967296.0);  // floor(p 2^32), p < 1
    P.keep_scale = 1.0f / (1.0f - a->dropout_p);
    return P;
}

// An entry point: everything is checked before anything is launched; launch(P) gets the filled common fields and adds its own.
// backward: grads is part of the call (and refused when null)
template <class Params, class Launch>
int attention_call(const char *fn, const AttnRules &rules, const AnceAttn16Args *args, bool backward, const AnceAttn16GradArgs *grads,
                   const uint64_t *d_stream, Launch launch) {
    if (!stream_aligned(d_stream)) return refuse(fn, "alignment: d_stream is not 16-byte aligned");
    if (const char *why = check_args(args, rules)) return refuse(fn, why);
    if (backward) {
        if (!grads) return refuse(fn, "null pointer");
        const int piece = piece_elems(args->dtype);
        if (const char *why = check_matrix(grads->dctx, grads->ld_dctx, args->n_heads, piece)) return refuse(fn, why);
        if (const char *why = check_matrix(grads->dq, grads->ld_dq, args->n_heads, piece)) return refuse(fn, why);
        if (const char *why = check_matrix(grads->dk, grads->ld_dk, args->n_heads, piece)) return refuse(fn, why);
        if (const char *why = check_matrix(grads->dv, grads->ld_dv, args->n_heads, piece)) return refuse(fn, why);
    }
    launch(params<Params>(args, backward ? grads : nullptr, d_stream));
    return check_launch(fn);
}

}  // namespace
}  // namespace ance
