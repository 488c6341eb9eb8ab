// The self-attention core for the FIRST query row of every sequence, with its gradient (include/ance_amd.h: ance_attention_row0_*):
// what a tower's last layer needs when only h[:, 0] is read.  Per sequence s (first row, len: seq_bounds) and head h of width 64,
// q0 = row s of the [n_seq, H] matrix q:
//   forward:  t_j = 0.125f * (q0 . K_j) for j < len;  m = max_j t_j;  l = sum_j expf(t_j - m);  P_j = expf(t_j - m) / l;
//             P'_j = keep_j ? P_j * keep_scale : 0;  ctx0 = sum_j P'_j V_j.  Saved: (m, l), two fp32 per (s, h); nothing of size L.
//   backward: t_j, P_j by the SAME expressions from the saved (m, l);  dP_j = keep_j ? (dctx0 . V_j) * keep_scale : 0;
//             D = sum_j dP_j P_j;  dS_j = P_j (dP_j - D);  dq0 = 0.125f sum_j dS_j K_j;  dK_j = 0.125f dS_j q0;  dV_j = P'_j dctx0;
//             rows len <= j < seq_rows of dK and dV are written as zeros; a sequence of length 0 writes a zero ctx0 and a zero dq0.
//   Dropout: the full core's row i = 0 (attention_train_kernels.h): Philox4x32-10, key (seed lo, seed hi), counter (j >> 2, s * n_heads + h,
//             offset lo, offset hi), word j & 3, keep iff word >= keep_thr.
// T = fp32, fp16 or bf16 is the type of the rows in memory only: all arithmetic is fp32, and every output element is rounded once at
// its store (to nearest even, overflow to +-inf: the plain conversion).  P is never rounded: there is no matrix operand here.
//
// The single-query pattern: a memory-bound pass over K and V, rows straight to registers in 16-byte pieces, no LDS tiling.  One
// workgroup of 256 threads per (sequence, head).  A row of 64 elements is LPR = 16 (fp32) or 8 (16-bit) pieces; a group of LPR
// adjacent lanes owns a row, so a wave reads 4 (8) whole rows at once, and the 256 threads walk the rows G = 256 / LPR at a time.
// Every sum has one owner and a fixed order: a dot product is an fmaf chain over the piece and an xor tree over the group; a sum
// over j is ascending in each group, then ascending over the groups; the workgroup's max / sum is an xor tree per wave, then the
// four waves in order.  No atomics: the same inputs give the same bits.  The grid comes from n_heads and n_seq; the lengths are
// read on the device; nothing waits for the host.
#include "attention_common.h"

namespace ance {
namespace {

constexpr int R0_THREADS = 256, R0_MAX_LEN = 512;

struct R0F32 {
    typedef float T;
    static constexpr int EPP = 4, LPR = 16;  // elements per 16-byte piece, pieces per 64-element row
    typedef float V __attribute__((ext_vector_type(4)));
};
struct R0F16 {
    typedef _Float16 T;
    static constexpr int EPP = 8, LPR = 8;
    typedef _Float16 V __attribute__((ext_vector_type(8)));
};
struct R0BF16 {
    typedef __bf16 T;
    static constexpr int EPP = 8, LPR = 8;
    typedef __bf16 V __attribute__((ext_vector_type(8)));
};

struct Row0Params {
    const void *q, *k, *v, *dctx;
    void *ctx, *dq, *dk, *dv;
    int64_t ld_q, ld_k, ld_v, ld_ctx, ld_dctx, ld_dq, ld_dk, ld_dv;
    const int32_t *seq_first, *seq_len;
    int max_seq_len, n_rows, n_heads, seq_rows;
    float *ml;  // [n_seq][n_heads][2]: max and sum (workspace)
    uint32_t seed_lo, seed_hi, off_lo, off_hi, keep_thr;
    float keep_scale;
    const uint64_t *d_stream;  // null, or the device stream {seed, base} (philox.h: drop_stream)
};

// piece c of row `row` (already at the head's columns) as fp32
template <class X>
__device__ __forceinline__ void load_piece(float out[X::EPP], const void *base, int64_t ld, int64_t row, int c) {
    const typename X::V p = *reinterpret_cast<const typename X::V *>((const typename X::T *)base + row * ld + c * X::EPP);
#pragma unroll
    for (int e = 0; e < X::EPP; ++e) out[e] = (float)p[e];
}
// the store of an output piece: each element rounded once, here
template <class X>
__device__ __forceinline__ void store_piece(void *base, int64_t ld, int64_t row, int c, const float in[X::EPP]) {
    typename X::V p;
#pragma unroll
    for (int e = 0; e < X::EPP; ++e) p[e] = (typename X::T)in[e];
    *reinterpret_cast<typename X::V *>((typename X::T *)base + row * ld + c * X::EPP) = p;
}

// a . b over a row: the fmaf chain over the lane's piece, then the xor tree over the row's LPR lanes (every lane gets the sum)
template <class X>
__device__ __forceinline__ float group_dot(const float a[X::EPP], const float b[X::EPP]) {
    float d = 0.f;
#pragma unroll
    for (int e = 0; e < X::EPP; ++e) d = __builtin_fmaf(a[e], b[e], d);
#pragma unroll
    for (int off = X::LPR / 2; off > 0; off >>= 1) d += __shfl_xor(d, off);
    return d;
}

// the workgroup's max / sum of one value per thread: xor tree per wave, then the four waves in order
template <bool MAX>
__device__ __forceinline__ float block_reduce(float x, float *red, int tid) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float y = __shfl_xor(x, off);
        x = MAX ? fmaxf(x, y) : x + y;
    }
    __syncthreads();  // red may still be read from the reduction before
    if ((tid & 63) == 0) red[tid >> 6] = x;
    __syncthreads();
    return MAX ? fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])) : ((red[0] + red[1]) + (red[2] + red[3]));
}

// t[j] = 0.125f * (q0 . K_j), j < len: ONE text for the forward and the backward, so that both see the same bits
template <class X>
__device__ __forceinline__ void scores(float *t, const Row0Params &P, const float qp[X::EPP], int64_t first, int len, int head, int g, int c) {
    constexpr int G = R0_THREADS / X::LPR;
    const typename X::T *kb = (const typename X::T *)P.k + 64 * head;
    for (int j = g; j < len; j += G) {
        float kp[X::EPP];
        load_piece<X>(kp, kb, P.ld_k, first + j, c);
        const float d = group_dot<X>(qp, kp);
        if (c == 0) t[j] = d * 0.125f;
    }
}

// keep bits of keys 4 j4 .. 4 j4 + 3 of (sequence s, head): bit e set = key 4 j4 + e is kept
template <int DROP>
__device__ __forceinline__ uint32_t keep4(const Row0Params &P, const DropStream &D, int s, int head, int j4) {
    if (!DROP) return 15u;
    uint32_t w[4];
    philox4((uint32_t)j4, (uint32_t)(s * P.n_heads + head), D.off_lo, D.off_hi, D.seed_lo, D.seed_hi, w);
    return (w[0] >= P.keep_thr ? 1u : 0u) | (w[1] >= P.keep_thr ? 2u : 0u) | (w[2] >= P.keep_thr ? 4u : 0u) | (w[3] >= P.keep_thr ? 8u : 0u);
}

// out[64] = scale * sum_j w[j] M_j over j < len, M the rows of `src` at the head's columns: ascending j in each group, then ascending
// groups; stored as row `orow` of dst.  part: [G][64] floats of LDS.
template <class X>
__device__ __forceinline__ void weighted_rows(float *part, const float *w, const void *src, int64_t ld, int64_t first, int len, int head,
                                              void *dst, int64_t ld_dst, int64_t orow, float scale, int tid) {
    constexpr int G = R0_THREADS / X::LPR;
    const int g = tid / X::LPR, c = tid % X::LPR;
    const typename X::T *sb = (const typename X::T *)src + 64 * head;
    float acc[X::EPP];
#pragma unroll
    for (int e = 0; e < X::EPP; ++e) acc[e] = 0.f;
#pragma unroll 4
    for (int j = g; j < len; j += G) {
        float mp[X::EPP];
        load_piece<X>(mp, sb, ld, first + j, c);
        const float wj = w[j];
#pragma unroll
        for (int e = 0; e < X::EPP; ++e) acc[e] = __builtin_fmaf(wj, mp[e], acc[e]);
    }
#pragma unroll
    for (int e = 0; e < X::EPP; ++e) part[g * 64 + c * X::EPP + e] = acc[e];
    __syncthreads();
    if (tid < X::LPR) {
        float out[X::EPP];
#pragma unroll
        for (int e = 0; e < X::EPP; ++e) {
            float sum = 0.f;
            for (int gg = 0; gg < G; ++gg) sum += part[gg * 64 + tid * X::EPP + e];
            out[e] = sum * scale;
        }
        store_piece<X>((typename X::T *)dst + 64 * head, ld_dst, orow, tid, out);
    }
}

template <class X>
__device__ __forceinline__ void zero_row0(void *dst, int64_t ld, int s, int head, int tid) {
    if (tid < X::LPR) {
        float z[X::EPP];
#pragma unroll
        for (int e = 0; e < X::EPP; ++e) z[e] = 0.f;
        store_piece<X>((typename X::T *)dst + 64 * head, ld, s, tid, z);
    }
}

template <class X, int DROP>
__global__ void __launch_bounds__(R0_THREADS) row0_fwd_kernel(const Row0Params P) {
    constexpr int G = R0_THREADS / X::LPR;
    __shared__ float t[R0_MAX_LEN], part[G * 64], red[4];
    const int head = blockIdx.x, s = blockIdx.y, tid = threadIdx.x;
    const int g = tid / X::LPR, c = tid % X::LPR;
    const DropStream D = drop_stream<DROP>(P);
    int first;
    const int len = seq_bounds(P, s, &first);
    if (len <= 0) {
        zero_row0<X>(P.ctx, P.ld_ctx, s, head, tid);
        return;
    }
    float qp[X::EPP];
    load_piece<X>(qp, (const typename X::T *)P.q + 64 * head, P.ld_q, s, c);
    scores<X>(t, P, qp, first, len, head, g, c);
    __syncthreads();
    float m = -INFINITY;
    for (int j = tid; j < len; j += R0_THREADS) m = fmaxf(m, t[j]);
    m = block_reduce<true>(m, red, tid);
    float l = 0.f;
    for (int j = tid; j < len; j += R0_THREADS) l += expf(t[j] - m);
    l = block_reduce<false>(l, red, tid);
    for (int j4 = tid; 4 * j4 < len; j4 += R0_THREADS) {
        const uint32_t keep = keep4<DROP>(P, D, s, head, j4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int j = 4 * j4 + e;
            if (j < len) {
                const float p = expf(t[j] - m) / l;
                t[j] = DROP ? ((keep >> e & 1u) ? p * P.keep_scale : 0.f) : p;  // P'
            }
        }
    }
    __syncthreads();
    weighted_rows<X>(part, t, P.v, P.ld_v, first, len, head, P.ctx, P.ld_ctx, s, 1.0f, tid);
    if (tid == 0) {
        float *ml = P.ml + 2 * ((int64_t)s * P.n_heads + head);
        ml[0] = m;
        ml[1] = l;
    }
}

template <class X, int DROP>
__global__ void __launch_bounds__(R0_THREADS) row0_bwd_kernel(const Row0Params P) {
    constexpr int G = R0_THREADS / X::LPR;
    __shared__ float t[R0_MAX_LEN], u[R0_MAX_LEN], part[G * 64], red[4];
    const int head = blockIdx.x, s = blockIdx.y, tid = threadIdx.x;
    const int g = tid / X::LPR, c = tid % X::LPR;
    const DropStream D = drop_stream<DROP>(P);
    int first;
    const int len = seq_bounds(P, s, &first);
    // the rows this sequence owns in dk / dv (the padded form): [0, own); none when its first row is outside the matrix
    int own = 0;
    if (P.seq_rows > 0 && first >= 0 && first < P.n_rows) own = P.seq_rows < P.n_rows - first ? P.seq_rows : P.n_rows - first;
    float qp[X::EPP], gp[X::EPP], z[X::EPP];
#pragma unroll
    for (int e = 0; e < X::EPP; ++e) z[e] = 0.f;
    typename X::T *dkb = (typename X::T *)P.dk + 64 * head, *dvb = (typename X::T *)P.dv + 64 * head;
    for (int j = (len > 0 ? len : 0) + g; j < own; j += G) {  // the pad rows' zeros
        store_piece<X>(dkb, P.ld_dk, (int64_t)first + j, c, z);
        store_piece<X>(dvb, P.ld_dv, (int64_t)first + j, c, z);
    }
    if (len <= 0) {
        zero_row0<X>(P.dq, P.ld_dq, s, head, tid);
        return;
    }
    load_piece<X>(qp, (const typename X::T *)P.q + 64 * head, P.ld_q, s, c);
    load_piece<X>(gp, (const typename X::T *)P.dctx + 64 * head, P.ld_dctx, s, c);
    scores<X>(t, P, qp, first, len, head, g, c);
    {  // u[j] = dctx0 . V_j
        const typename X::T *vb = (const typename X::T *)P.v + 64 * head;
        for (int j = g; j < len; j += G) {
            float vp[X::EPP];
            load_piece<X>(vp, vb, P.ld_v, (int64_t)first + j, c);
            const float d = group_dot<X>(gp, vp);
            if (c == 0) u[j] = d;
        }
    }
    __syncthreads();
    const float *ml = P.ml + 2 * ((int64_t)s * P.n_heads + head);
    const float m = ml[0], l = ml[1];
    // t[j] <- P_j, u[j] <- dP_j; each thread keeps the keep bits of its quads for the second pass
    float dsum = 0.f;
    for (int j4 = tid; 4 * j4 < len; j4 += R0_THREADS) {
        const uint32_t keep = keep4<DROP>(P, D, s, head, j4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int j = 4 * j4 + e;
            if (j < len) {
                const float p = expf(t[j] - m) / l;
                const float dp = DROP ? ((keep >> e & 1u) ? u[j] * P.keep_scale : 0.f) : u[j];
                t[j] = p;
                u[j] = dp;
                dsum = __builtin_fmaf(dp, p, dsum);
            }
        }
    }
    const float Dr = block_reduce<false>(dsum, red, tid);
    // t[j] <- dS_j, u[j] <- P'_j (the same thread owns the same quads: no barrier in between)
    for (int j4 = tid; 4 * j4 < len; j4 += R0_THREADS) {
        const uint32_t keep = keep4<DROP>(P, D, s, head, j4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int j = 4 * j4 + e;
            if (j < len) {
                const float p = t[j];
                t[j] = p * (u[j] - Dr);
                u[j] = DROP ? ((keep >> e & 1u) ? p * P.keep_scale : 0.f) : p;
            }
        }
    }
    __syncthreads();
    for (int j = g; j < len; j += G) {  // dK_j = 0.125 dS_j q0, dV_j = P'_j dctx0
        const float ds = t[j] * 0.125f, pk = u[j];
        float a[X::EPP], b[X::EPP];
#pragma unroll
        for (int e = 0; e < X::EPP; ++e) {
            a[e] = ds * qp[e];
            b[e] = pk * gp[e];
        }
        store_piece<X>(dkb, P.ld_dk, (int64_t)first + j, c, a);
        store_piece<X>(dvb, P.ld_dv, (int64_t)first + j, c, b);
    }
    weighted_rows<X>(part, t, P.k, P.ld_k, first, len, head, P.dq, P.ld_dq, s, 0.125f, tid);  // dq0 = 0.125 sum_j dS_j K_j
}

template <class X, bool BWD>
void launch(const AnceAttn16Args *args, const Row0Params &P, hipStream_t st) {
    const dim3 grid((unsigned)args->n_heads, (unsigned)args->n_seq), block(R0_THREADS);
    const int mode = drop_mode(drops(args), P.d_stream);
    if (BWD) {
        if (mode == DROP_DEVICE) hipLaunchKernelGGL((row0_bwd_kernel<X, DROP_DEVICE>), grid, block, 0, st, P);
        else if (mode == DROP_HOST) hipLaunchKernelGGL((row0_bwd_kernel<X, DROP_HOST>), grid, block, 0, st, P);
        else hipLaunchKernelGGL((row0_bwd_kernel<X, DROP_NONE>), grid, block, 0, st, P);
    } else {
        if (mode == DROP_DEVICE) hipLaunchKernelGGL((row0_fwd_kernel<X, DROP_DEVICE>), grid, block, 0, st, P);
        else if (mode == DROP_HOST) hipLaunchKernelGGL((row0_fwd_kernel<X, DROP_HOST>), grid, block, 0, st, P);
        else hipLaunchKernelGGL((row0_fwd_kernel<X, DROP_NONE>), grid, block, 0, st, P);
    }
}
template <bool BWD>
void launch_typed(const AnceAttn16Args *args, const Row0Params &P, hipStream_t st) {
    if (args->dtype == ANCE_DTYPE_F16) launch<R0F16, BWD>(args, P, st);
    else if (args->dtype == ANCE_DTYPE_BF16) launch<R0BF16, BWD>(args, P, st);
    else launch<R0F32, BWD>(args, P, st);
}

size_t ws_bytes(int64_t n_seq, int n_heads) { return align_up(2 * sizeof(float) * (size_t)n_seq * (size_t)n_heads, 256); }

// an entry point: attention_call with all three dtypes and the workspace as (max, sum) per (sequence, head)
template <bool BWD>
int call(const char *fn, const AnceAttn16Args *args, const AnceAttn16GradArgs *grads, const uint64_t *d_stream, void *stream) {
    const AttnRules rules = {1u << ANCE_DTYPE_F32 | 1u << ANCE_DTYPE_F16 | 1u << ANCE_DTYPE_BF16, "dtype not ANCE_DTYPE_F32, _F16 or _BF16",
                             args ? ws_bytes(args->n_seq, args->n_heads) : 0};
    return attention_call<Row0Params>(fn, rules, args, BWD, grads, d_stream, [&](Row0Params P) {
        P.ml = (float *)args->d_workspace;
        launch_typed<BWD>(args, P, (hipStream_t)stream);
    });
}

}  // namespace
}  // namespace ance

extern "C" size_t ance_attention_row0_workspace_bytes(int64_t n_seq, int n_heads) {
    return ance::shape_ok(n_seq, 65535, n_heads) ? ance::ws_bytes(n_seq, n_heads) : 0;
}

// The entry points: each with its sibling that takes the device dropout stream (include/ance_amd.h); the plain one passes none.
extern "C" int ance_attention_row0_forward(const AnceAttn16Args *args, void *stream) {
    return ance::call<false>("ance_attention_row0_forward", args, nullptr, nullptr, stream);
}
extern "C" int ance_attention_row0_forward_dstream(const AnceAttn16Args *args, const uint64_t *d_stream, void *stream) {
    return ance::call<false>("ance_attention_row0_forward_dstream", args, nullptr, d_stream, stream);
}
extern "C" int ance_attention_row0_backward(const AnceAttn16Args *args, const AnceAttn16GradArgs *grads, void *stream) {
    return ance::call<true>("ance_attention_row0_backward", args, grads, nullptr, stream);
}
extern "C" int ance_attention_row0_backward_dstream(const AnceAttn16Args *args, const AnceAttn16GradArgs *grads, const uint64_t *d_stream,
                                                    void *stream) {
    return ance::call<true>("ance_attention_row0_backward_dstream", args, grads, d_stream, stream);
}
