// The trainers' self-attention core in 16-bit I/O (include/ance_amd.h: ance_attention16_forward / ance_attention16_backward): the
// mathematics, the padded and packed forms, the pad-row zeros, the workspace and the dropout stream of attention_train.hip, with q, k,
// v, ctx, dctx, dq, dk, dv as fp16 or bf16 rows and every product on the 16-bit matrix cores (v_mfma_f32_32x32x16_f16 / _bf16).
//
// The arithmetic contract (T = the I/O type; "rounded" = to nearest even, overflow to +-inf: the plain conversion, v_cvt_f16_f32 /
// v_cvt_pk_bf16_f32 -- never a truncating or saturating form: under a GradScaler an overflowing dS has to arrive as inf, not clamped):
//   S = Q K^T with T operands and fp32 accumulation; t = S * 0.125f in fp32; pad keys are skipped (t = -inf).
//   ex(x) = exp2(x * log2 e) on the hardware exp2 (v_exp_f32): ONE expression, used by the forward and by both backward kernels.
//   forward: online softmax over ascending 32-key blocks, max / exp / sum in fp32: e = ex(t - m_running); the row's sum takes the
//     unrounded e; P' = keep o e is rounded to T for ctx^T += V^T P'^T; ctx accumulates in fp32 over all blocks (rescaled by
//     ex(m_old - m_new) in fp32) and is rounded once at the store, after the fp32 factor (1.0f / (1.0f - p)) / sum.
//     lse = m + logf(sum), one fp32 per (head, row), in the workspace as [n_heads][n_rows]; behind it [n_heads][n_rows] of D.
//   backward 1: P = ex(t - lse) with t recomputed by the SAME expression (the same products in the same MFMA, operands swapped at
//     most, scaled by 0.125f in fp32): a saturated row's P must not move by ulp(S) between the passes.
//   backward 2: D = dctx . ctx in fp32 from the stored (rounded) ctx.
//   backward 3: dP = dctx V^T accumulates in fp32; dropout: dP = keep ? dP * (1.0f / (1.0f - p)) : 0 in fp32.
//   backward 4: dS = P o (dP - D) in fp32, rounded to T for dQ^T += K^T dS^T and dK^T += Q^T dS; P' = keep ? P * (1.0f / (1.0f - p))
//     : 0 rounded to T for dV^T += dctx^T P'.
//   backward 5: dq, dk, dv accumulate in fp32 registers under one owning workgroup per 64-row tile, blocks in ascending order; dq and
//     dk are scaled by 0.125f in fp32; each is rounded once at the store.
//   Dropout: the Philox counter and keep rule of attention_train.hip, unchanged: (seed, offset, s, h, i, j) keeps the same element.
//
// Operand maps.  v_mfma_f32_32x32x16: lane l (r = l & 31, h = l >> 5) holds A[r][8h + j] and B[8h + j][r] in element j of its
// 8-element fragment; C/D is that of every 32x32 MFMA: column l & 31, rows 8a + 4h + b in register 4a + b.
//   "rows" product  acc[m][n] = sum_d blk[m][d] own[n][d]  (S, S^T, dP, dP^T): k-step t is d = 16t + 8h + j.  A = 16 bytes of row m
//     of the block's ROW image in LDS ([32][72] T: 144-byte rows), B = 16 bytes of the lane's own row, loaded once from memory.
//   "cols" product  acc[d][n] += sum_r blk[r][d] X[r][n]  with X a C/D-layout block left in its registers (P', dS): registers
//     8s .. 8s + 7 converted to T ARE the B fragment of k-step s, which permutes k inside the step: element j of half h is block row
//     16s + 8(j >> 2) + 4h + (j & 3).  The A fragment follows that order: elements 0..3 = blkT[d][16s + 4h ..], 4..7 =
//     blkT[d][16s + 8 + 4h ..]: two 8-byte reads of the block's TRANSPOSED image ([64][36] T: 72-byte rows, conflict-free), which
//     the staging threads write as (row 2u, row 2u + 1) pairs, one 4-byte store per column.
// A workgroup is two waves on a 64-row tile, as in the fp32 file; the other side comes in 32-row blocks.
#include "common.h"
#include "philox.h"
#include "attention_train.h"

namespace ance {
namespace {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x2 __attribute__((ext_vector_type(2)));

struct F16 {
    typedef _Float16 T;
    typedef _Float16 V8 __attribute__((ext_vector_type(8)));
    typedef _Float16 V4 __attribute__((ext_vector_type(4)));
    typedef _Float16 V2 __attribute__((ext_vector_type(2)));
    static __device__ __forceinline__ f32x16 mfma(V8 a, V8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }
};
struct BF16 {
    typedef __bf16 T;
    typedef __bf16 V8 __attribute__((ext_vector_type(8)));
    typedef __bf16 V4 __attribute__((ext_vector_type(4)));
    typedef __bf16 V2 __attribute__((ext_vector_type(2)));
    static __device__ __forceinline__ f32x16 mfma(V8 a, V8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
};

constexpr int AH_THREADS = 128, AH_TILE = 64, AH_BLK = 32;
constexpr int AH_LDR = 72;  // row image [32][72]: 144-byte rows, 16-byte aligned
constexpr int AH_LDT = 36;  // transposed image [64][36]: 72-byte rows, 8-byte aligned; 18 banks a row: 32 rows x 2 banks, all distinct
constexpr float LOG2E = 1.4426950408889634f;

struct AttnParams16 {
    const void *q, *k, *v, *ctx, *dctx;
    void *ctx_out, *dq, *dk, *dv;
    int64_t ld_q, ld_k, ld_v, ld_ctx, ld_dctx, ld_dq, ld_dk, ld_dv;
    const int32_t *seq_first, *seq_len;
    int max_seq_len, n_rows, n_heads, seq_rows;
    float *lse, *rowdot;  // [n_heads][n_rows] each (workspace)
    uint32_t seed_lo, seed_hi, off_lo, off_hi, keep_thr;
    float keep_scale;
    const uint64_t *d_stream;  // null, or the device stream {seed, base} (philox.h: drop_stream)
};

// the one exp of this file: the forward and both backward kernels
__device__ __forceinline__ float ex(float x) { return __builtin_amdgcn_exp2f(x * LOG2E); }

template <class X>
__device__ __forceinline__ typename X::V8 zero8() {
    return __builtin_bit_cast(typename X::V8, i32x4{0, 0, 0, 0});
}

// the pad rows of the padded form: rows [max(t0, len), min(t0 + 64, own)) of the head's 64 columns of dst, as zeros (attention_train.hip)
template <class X>
__device__ __forceinline__ void zero_pad_rows(const AttnParams16 &P, typename X::T *dst, int64_t ld, int first, int len, int t0, int tid) {
    if (P.seq_rows <= 0 || first < 0 || first >= P.n_rows) return;
    const int own = P.seq_rows < P.n_rows - first ? P.seq_rows : P.n_rows - first;
    const int lo = t0 > len ? t0 : len, hi = t0 + AH_TILE < own ? t0 + AH_TILE : own;
    for (int e = tid; e < (hi - lo) * 8; e += AH_THREADS)
        *reinterpret_cast<typename X::V8 *>(dst + ((int64_t)first + lo + (e >> 3)) * ld + (e & 7) * 8) = zero8<X>();
}

// 32 rows x 64 elements from row0 of src (already at the head's columns): thread (u = tid >> 3, ch = tid & 7) carries the 16-byte
// chunk ch of rows 2u and 2u + 1 (rows >= valid are zeros, never read from memory)
template <class X>
struct Stage {
    typename X::V8 a, b;
};
template <class X>
__device__ __forceinline__ void fetch_block(Stage<X> *st, const typename X::T *src, int64_t ld, int64_t row0, int valid, int tid) {
    const int u = tid >> 3, ch = tid & 7;
    st->a = zero8<X>();
    st->b = zero8<X>();
    if (2 * u < valid) st->a = *reinterpret_cast<const typename X::V8 *>(src + (row0 + 2 * u) * ld + 8 * ch);
    if (2 * u + 1 < valid) st->b = *reinterpret_cast<const typename X::V8 *>(src + (row0 + 2 * u + 1) * ld + 8 * ch);
}
template <class X>
__device__ __forceinline__ void put_rows(typename X::T *dst, const Stage<X> &st, int tid) {  // dst [32][AH_LDR]
    const int u = tid >> 3, ch = tid & 7;
    *reinterpret_cast<typename X::V8 *>(dst + (2 * u) * AH_LDR + 8 * ch) = st.a;
    *reinterpret_cast<typename X::V8 *>(dst + (2 * u + 1) * AH_LDR + 8 * ch) = st.b;
}
template <class X>
__device__ __forceinline__ void put_cols(typename X::T *dst, const Stage<X> &st, int tid) {  // dst [64][AH_LDT]: dst[d][r] = block[r][d]
    const int u = tid >> 3, ch = tid & 7;
#pragma unroll
    for (int e = 0; e < 8; ++e)
        *reinterpret_cast<typename X::V2 *>(dst + (8 * ch + e) * AH_LDT + 2 * u) = typename X::V2{st.a[e], st.b[e]};
}

// the lane's own row as the B fragments of the four k-steps: reg[t] = row[16t + 8 half .. + 7]; zeros for a row that is not valid
template <class X>
__device__ __forceinline__ void load_row_frags(typename X::V8 reg[4], const typename X::T *src, int64_t ld, int64_t row, bool valid, int half) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        reg[t] = zero8<X>();
        if (valid) reg[t] = *reinterpret_cast<const typename X::V8 *>(src + row * ld + 16 * t + 8 * half);
    }
}

// acc[m][n] += sum_d blk[m = l & 31][d] reg[n = l & 31][d]: the row image supplies A, the lane's own row B
template <class X>
__device__ __forceinline__ f32x16 mma_block_rows(const typename X::T *blk, const typename X::V8 reg[4], int lane, f32x16 acc) {
    const typename X::T *row = blk + (lane & 31) * AH_LDR + 8 * (lane >> 5);
#pragma unroll
    for (int t = 0; t < 4; ++t) acc = X::mfma(*reinterpret_cast<const typename X::V8 *>(row + 16 * t), reg[t], acc);
    return acc;
}

// a C/D-layout fp32 block, rounded to T, as the two B fragments of the next product (k = its row index, permuted inside a step)
template <class X>
__device__ __forceinline__ void pack_block(const f32x16 x, typename X::V8 out[2]) {
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int j = 0; j < 8; ++j) out[s][j] = (typename X::T)x[8 * s + j];
}

// acc0[d][n] += sum_r blkT[d][r] b[r][n], acc1 the same for d + 32: A from the transposed image in the k order of pack_block
template <class X>
__device__ __forceinline__ void mma_block_cols(const typename X::T *blkT, const typename X::V8 b[2], int lane, f32x16 *acc0, f32x16 *acc1) {
    const typename X::T *col = blkT + (lane & 31) * AH_LDT + 4 * (lane >> 5);
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const typename X::V4 lo0 = *reinterpret_cast<const typename X::V4 *>(col + 16 * s);
        const typename X::V4 hi0 = *reinterpret_cast<const typename X::V4 *>(col + 16 * s + 8);
        const typename X::V4 lo1 = *reinterpret_cast<const typename X::V4 *>(col + 32 * AH_LDT + 16 * s);
        const typename X::V4 hi1 = *reinterpret_cast<const typename X::V4 *>(col + 32 * AH_LDT + 16 * s + 8);
        *acc0 = X::mfma(__builtin_shufflevector(lo0, hi0, 0, 1, 2, 3, 4, 5, 6, 7), b[s], *acc0);
        *acc1 = X::mfma(__builtin_shufflevector(lo1, hi1, 0, 1, 2, 3, 4, 5, 6, 7), b[s], *acc1);
    }
}

// a C/D-layout accumulator pair (rows = head columns d, column = the lane's own row) -> 64 elements of the lane's row: times scale
// in fp32, then rounded once
template <class X>
__device__ __forceinline__ void store_row_t(typename X::T *dst, const f32x16 acc0, const f32x16 acc1, int half, float scale) {
    typedef typename X::T T;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        *reinterpret_cast<typename X::V4 *>(dst + 8 * a + 4 * half) = typename X::V4{
            (T)(acc0[4 * a] * scale), (T)(acc0[4 * a + 1] * scale), (T)(acc0[4 * a + 2] * scale), (T)(acc0[4 * a + 3] * scale)};
        *reinterpret_cast<typename X::V4 *>(dst + 32 + 8 * a + 4 * half) = typename X::V4{
            (T)(acc1[4 * a] * scale), (T)(acc1[4 * a + 1] * scale), (T)(acc1[4 * a + 2] * scale), (T)(acc1[4 * a + 3] * scale)};
    }
}

template <class X, int DROP>
__global__ void __launch_bounds__(AH_THREADS) attn16_fwd_kernel(const AttnParams16 P) {
    typedef typename X::T T;
    __shared__ __attribute__((aligned(16))) T Ks[AH_BLK * AH_LDR], Vt[64 * AH_LDT];
    const int s = blockIdx.z, head = blockIdx.y, q0 = blockIdx.x * AH_TILE;
    const DropStream D = drop_stream<DROP>(P);
    int first;
    const int len = seq_bounds(P, s, &first);
    zero_pad_rows<X>(P, (T *)P.ctx_out + 64 * head, P.ld_ctx, first, len, q0, threadIdx.x);
    if (q0 >= len) return;
    const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5;
    const int qi = q0 + 32 * (tid >> 6) + (lane & 31);
    const bool qok = qi < len;
    const int64_t qrow = (int64_t)first + qi;
    typename X::V8 qreg[4];
    load_row_frags<X>(qreg, (const T *)P.q + 64 * head, P.ld_q, qrow, qok, half);
    const T *kbase = (const T *)P.k + 64 * head, *vbase = (const T *)P.v + 64 * head;
    f32x16 acc0 = {}, acc1 = {};
    float m = -INFINITY, l = 0.f;
    Stage<X> kn, vn;
    fetch_block<X>(&kn, kbase, P.ld_k, (int64_t)first, len, tid);
    fetch_block<X>(&vn, vbase, P.ld_v, (int64_t)first, len, tid);
    for (int jb = 0; jb < len; jb += AH_BLK) {
        __syncthreads();
        put_rows<X>(Ks, kn, tid);
        put_cols<X>(Vt, vn, tid);
        __syncthreads();
        if (jb + AH_BLK < len) {  // the next block's loads travel while this block is multiplied
            fetch_block<X>(&kn, kbase, P.ld_k, (int64_t)first + jb + AH_BLK, len - jb - AH_BLK, tid);
            fetch_block<X>(&vn, vbase, P.ld_v, (int64_t)first + jb + AH_BLK, len - jb - AH_BLK, tid);
        }
        f32x16 sc = {};
        sc = mma_block_rows<X>(Ks, qreg, lane, sc);  // S^T: rows = keys, column = this lane's query
        float mb = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int j = jb + 8 * (r >> 2) + 4 * half + (r & 3);
            sc[r] = j < len ? sc[r] * 0.125f : -INFINITY;
            mb = fmaxf(mb, sc[r]);
        }
        mb = fmaxf(mb, __shfl_xor(mb, 32));
        const float mn = fmaxf(m, mb);  // finite: key 0 is valid and sits in the first block
        const float alpha = ex(m - mn);
        float sum = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            sc[r] = ex(sc[r] - mn);
            sum += sc[r];
        }
        sum += __shfl_xor(sum, 32);
        l = l * alpha + sum;
        m = mn;
        if (DROP) {
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                uint32_t w[4];
                philox4((uint32_t)qi * 128u + (uint32_t)((jb + 8 * a + 4 * half) >> 2), (uint32_t)(s * P.n_heads + head), D.off_lo, D.off_hi,
                        D.seed_lo, D.seed_hi, w);
#pragma unroll
                for (int e = 0; e < 4; ++e) sc[4 * a + e] = w[e] >= P.keep_thr ? sc[4 * a + e] : 0.f;
            }
        }
        typename X::V8 pb[2];
        pack_block<X>(sc, pb);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            acc0[r] *= alpha;
            acc1[r] *= alpha;
        }
        mma_block_cols<X>(Vt, pb, lane, &acc0, &acc1);  // ctx^T: rows = d, column = this lane's query
    }
    if (qok) {
        const float inv = (DROP ? P.keep_scale : 1.0f) / l;
        store_row_t<X>((T *)P.ctx_out + qrow * P.ld_ctx + 64 * head, acc0, acc1, half, inv);
        if (half == 0) P.lse[(int64_t)head * P.n_rows + qrow] = m + logf(l);
    }
}

// D[head][row] = dctx[row] . ctx[row] over the head's 64 columns in fp32: 8 lanes per (row, head), fixed xor tree
template <class X>
__global__ void __launch_bounds__(256) attn16_rowdot_kernel(const AttnParams16 P) {
    typedef typename X::T T;
    const int s = blockIdx.z, head = blockIdx.y;
    int first;
    const int len = seq_bounds(P, s, &first);
    const int i = blockIdx.x * 32 + (threadIdx.x >> 3), c = (threadIdx.x & 7) * 8;
    if (blockIdx.x * 32 >= len) return;
    const bool ok = i < len;
    const int64_t row = (int64_t)first + i;
    float d = 0.f;
    if (ok) {
        const typename X::V8 a = *reinterpret_cast<const typename X::V8 *>((const T *)P.dctx + row * P.ld_dctx + 64 * head + c);
        const typename X::V8 b = *reinterpret_cast<const typename X::V8 *>((const T *)P.ctx + row * P.ld_ctx + 64 * head + c);
#pragma unroll
        for (int e = 0; e < 8; ++e) d = __builtin_fmaf((float)a[e], (float)b[e], d);
    }
#pragma unroll
    for (int off = 4; off > 0; off >>= 1) d += __shfl_xor(d, off);
    if (ok && c == 0) P.rowdot[(int64_t)head * P.n_rows + row] = d;
}

template <class X, int DROP>
__global__ void __launch_bounds__(AH_THREADS) attn16_dq_kernel(const AttnParams16 P) {
    typedef typename X::T T;
    __shared__ __attribute__((aligned(16))) T Ks[AH_BLK * AH_LDR], Vs[AH_BLK * AH_LDR], Kt[64 * AH_LDT];
    const int s = blockIdx.z, head = blockIdx.y, q0 = blockIdx.x * AH_TILE;
    const DropStream D = drop_stream<DROP>(P);
    int first;
    const int len = seq_bounds(P, s, &first);
    zero_pad_rows<X>(P, (T *)P.dq + 64 * head, P.ld_dq, first, len, q0, threadIdx.x);
    if (q0 >= len) return;
    const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5;
    const int qi = q0 + 32 * (tid >> 6) + (lane & 31);
    const bool qok = qi < len;
    const int64_t qrow = (int64_t)first + qi;
    typename X::V8 qreg[4], greg[4];
    load_row_frags<X>(qreg, (const T *)P.q + 64 * head, P.ld_q, qrow, qok, half);
    load_row_frags<X>(greg, (const T *)P.dctx + 64 * head, P.ld_dctx, qrow, qok, half);
    const float lse = qok ? P.lse[(int64_t)head * P.n_rows + qrow] : 0.f;
    const float rd = qok ? P.rowdot[(int64_t)head * P.n_rows + qrow] : 0.f;
    const T *kbase = (const T *)P.k + 64 * head, *vbase = (const T *)P.v + 64 * head;
    f32x16 acc0 = {}, acc1 = {};
    Stage<X> kn, vn;
    fetch_block<X>(&kn, kbase, P.ld_k, (int64_t)first, len, tid);
    fetch_block<X>(&vn, vbase, P.ld_v, (int64_t)first, len, tid);
    for (int jb = 0; jb < len; jb += AH_BLK) {
        __syncthreads();
        put_rows<X>(Ks, kn, tid);
        put_cols<X>(Kt, kn, tid);
        put_rows<X>(Vs, vn, tid);
        __syncthreads();
        if (jb + AH_BLK < len) {  // the next block's loads travel while this block is multiplied
            fetch_block<X>(&kn, kbase, P.ld_k, (int64_t)first + jb + AH_BLK, len - jb - AH_BLK, tid);
            fetch_block<X>(&vn, vbase, P.ld_v, (int64_t)first + jb + AH_BLK, len - jb - AH_BLK, tid);
        }
        f32x16 sc = {}, dp = {};
        sc = mma_block_rows<X>(Ks, qreg, lane, sc);  // S^T
        dp = mma_block_rows<X>(Vs, greg, lane, dp);  // dP^T = V dctx^T
        uint32_t w[16];
        if (DROP) {
#pragma unroll
            for (int a = 0; a < 4; ++a)
                philox4((uint32_t)qi * 128u + (uint32_t)((jb + 8 * a + 4 * half) >> 2), (uint32_t)(s * P.n_heads + head), D.off_lo, D.off_hi,
                        D.seed_lo, D.seed_hi, w + 4 * a);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int j = jb + 8 * (r >> 2) + 4 * half + (r & 3);
            const float p = (j < len && qok) ? ex(sc[r] * 0.125f - lse) : 0.f;
            float g = dp[r];
            if (DROP) g = w[r] >= P.keep_thr ? g * P.keep_scale : 0.f;
            sc[r] = p * (g - rd);  // dS^T
        }
        typename X::V8 db[2];
        pack_block<X>(sc, db);
        mma_block_cols<X>(Kt, db, lane, &acc0, &acc1);  // dQ^T += K^T dS^T
    }
    if (qok) store_row_t<X>((T *)P.dq + qrow * P.ld_dq + 64 * head, acc0, acc1, half, 0.125f);
}

template <class X, int DROP>
__global__ void __launch_bounds__(AH_THREADS) attn16_dkv_kernel(const AttnParams16 P) {
    typedef typename X::T T;
    __shared__ __attribute__((aligned(16))) T Qs[AH_BLK * AH_LDR], Gs[AH_BLK * AH_LDR], Qt[64 * AH_LDT], Gt[64 * AH_LDT];
    __shared__ __attribute__((aligned(16))) float lse_s[AH_BLK], rd_s[AH_BLK];
    const int s = blockIdx.z, head = blockIdx.y, k0 = blockIdx.x * AH_TILE;
    const DropStream D = drop_stream<DROP>(P);
    int first;
    const int len = seq_bounds(P, s, &first);
    zero_pad_rows<X>(P, (T *)P.dk + 64 * head, P.ld_dk, first, len, k0, threadIdx.x);
    zero_pad_rows<X>(P, (T *)P.dv + 64 * head, P.ld_dv, first, len, k0, threadIdx.x);
    if (k0 >= len) return;
    const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5;
    const int kj = k0 + 32 * (tid >> 6) + (lane & 31);
    const bool kok = kj < len;
    const int64_t krow = (int64_t)first + kj;
    typename X::V8 kreg[4], vreg[4];
    load_row_frags<X>(kreg, (const T *)P.k + 64 * head, P.ld_k, krow, kok, half);
    load_row_frags<X>(vreg, (const T *)P.v + 64 * head, P.ld_v, krow, kok, half);
    const T *qbase = (const T *)P.q + 64 * head, *gbase = (const T *)P.dctx + 64 * head;
    f32x16 ak0 = {}, ak1 = {}, av0 = {}, av1 = {};
    Stage<X> qn, gn;
    fetch_block<X>(&qn, qbase, P.ld_q, (int64_t)first, len, tid);
    fetch_block<X>(&gn, gbase, P.ld_dctx, (int64_t)first, len, tid);
    for (int ib = 0; ib < len; ib += AH_BLK) {
        __syncthreads();
        put_rows<X>(Qs, qn, tid);
        put_cols<X>(Qt, qn, tid);
        put_rows<X>(Gs, gn, tid);
        put_cols<X>(Gt, gn, tid);
        if (tid < AH_BLK) {
            const bool ok = ib + tid < len;
            const int64_t o = (int64_t)head * P.n_rows + first + ib + tid;
            lse_s[tid] = ok ? P.lse[o] : 0.f;
            rd_s[tid] = ok ? P.rowdot[o] : 0.f;
        }
        __syncthreads();
        if (ib + AH_BLK < len) {  // the next block's loads travel while this block is multiplied
            fetch_block<X>(&qn, qbase, P.ld_q, (int64_t)first + ib + AH_BLK, len - ib - AH_BLK, tid);
            fetch_block<X>(&gn, gbase, P.ld_dctx, (int64_t)first + ib + AH_BLK, len - ib - AH_BLK, tid);
        }
        f32x16 sc = {}, dp = {};
        sc = mma_block_rows<X>(Qs, kreg, lane, sc);  // S: rows = queries, column = this lane's key
        dp = mma_block_rows<X>(Gs, vreg, lane, dp);  // dP = dctx V^T
        f32x16 pd;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const f32x4 ls = *reinterpret_cast<const f32x4 *>(lse_s + 8 * a + 4 * half), rd = *reinterpret_cast<const f32x4 *>(rd_s + 8 * a + 4 * half);
            uint32_t wj[4];
            if (DROP) {
                // The four lanes of a quad hold keys 4t .. 4t + 3: one counter per query row serves all four.  Lane c of the quad
                // draws for row c of this group of four rows; every lane then takes word c (its key's) of each row's draw.
                const int c = lane & 3;  // == kj & 3: k0 and the wave's offset are multiples of 4
                uint32_t w[4];
                philox4((uint32_t)(ib + 8 * a + 4 * half + c) * 128u + (uint32_t)(kj >> 2), (uint32_t)(s * P.n_heads + head), D.off_lo,
                        D.off_hi, D.seed_lo, D.seed_hi, w);
                wj[0] = quad_word<0>(w, c);
                wj[1] = quad_word<1>(w, c);
                wj[2] = quad_word<2>(w, c);
                wj[3] = quad_word<3>(w, c);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int r = 4 * a + e, i = ib + 8 * a + 4 * half + e;
                const float p = (i < len && kok) ? ex(sc[r] * 0.125f - ls[e]) : 0.f;
                float g = dp[r], pk = p;
                if (DROP) {
                    const bool keep = wj[e] >= P.keep_thr;
                    g = keep ? g * P.keep_scale : 0.f;
                    pk = keep ? p * P.keep_scale : 0.f;
                }
                pd[r] = pk;               // P'
                sc[r] = p * (g - rd[e]);  // dS
            }
        }
        typename X::V8 pb[2], db[2];
        pack_block<X>(pd, pb);
        pack_block<X>(sc, db);
        mma_block_cols<X>(Gt, pb, lane, &av0, &av1);  // dV^T += dctx^T P'
        mma_block_cols<X>(Qt, db, lane, &ak0, &ak1);  // dK^T += Q^T dS
    }
    if (kok) {
        store_row_t<X>((T *)P.dk + krow * P.ld_dk + 64 * head, ak0, ak1, half, 0.125f);
        store_row_t<X>((T *)P.dv + krow * P.ld_dv + 64 * head, av0, av1, half, 1.0f);
    }
}

int refuse(const char *fn, const char *why) {
    char buf[200];
    snprintf(buf, sizeof(buf), "%s: invalid argument (%s)", fn, why);
    set_last_error(buf);
    return ANCE_E_INVALID;
}
bool shape_ok(int64_t n_rows, int n_heads) { return n_rows >= 1 && n_rows <= 0x7fffffff && (n_heads == 12 || n_heads == 16); }
size_t ws_bytes(int64_t n_rows, int n_heads) { return 2 * align_up(sizeof(float) * (size_t)n_rows * (size_t)n_heads, 256); }
const char *check_matrix(const void *p, int ld, int n_heads) {
    if (!p) return "null pointer";
    if ((uintptr_t)p % 16) return "alignment: a base is not 16-byte aligned";
    if (ld % 8 != 0 || ld < 64 * n_heads) return "stride: not a multiple of 8 or below 64 * n_heads";
    return nullptr;
}
const char *check_args(const AnceAttn16Args *a) {
    if (!a) return "null pointer";
    if (a->dtype != ANCE_DTYPE_F16 && a->dtype != ANCE_DTYPE_BF16) return "dtype not ANCE_DTYPE_F16 or ANCE_DTYPE_BF16";
    if (a->n_heads != 12 && a->n_heads != 16) return "n_heads not 12 or 16";
    if (a->max_seq_len < 1 || a->max_seq_len > 512) return "max_seq_len outside 1 .. 512";
    if (a->n_seq < 1 || a->n_seq > 65535) return "n_seq outside 1 .. 65535";
    if (a->n_rows < 1) return "n_rows < 1";
    if (a->seq_rows < 0 || a->seq_rows > a->max_seq_len) return "seq_rows outside 0 .. max_seq_len";
    if (!a->d_seq_first || !a->d_seq_len) return "null pointer";
    if (const char *why = check_matrix(a->q, a->ld_q, a->n_heads)) return why;
    if (const char *why = check_matrix(a->k, a->ld_k, a->n_heads)) return why;
    if (const char *why = check_matrix(a->v, a->ld_v, a->n_heads)) return why;
    if (const char *why = check_matrix(a->ctx, a->ld_ctx, a->n_heads)) return why;
    if (!(a->dropout_p >= 0.0f && a->dropout_p < 1.0f)) return "dropout_p outside [0, 1)";
    if (!a->d_workspace || (uintptr_t)a->d_workspace % 16) return "null or unaligned workspace";
    if (a->workspace_bytes < ws_bytes(a->n_rows, a->n_heads)) return "workspace too small";
    return nullptr;
}
AttnParams16 params(const AnceAttn16Args *a, const uint64_t *d_stream) {
    AttnParams16 P = {};
    P.q = a->q; P.k = a->k; P.v = a->v; P.ctx = a->ctx; P.ctx_out = a->ctx;
    P.ld_q = a->ld_q; P.ld_k = a->ld_k; P.ld_v = a->ld_v; P.ld_ctx = a->ld_ctx;
    P.seq_first = a->d_seq_first; P.seq_len = a->d_seq_len;
    P.max_seq_len = a->max_seq_len; P.n_rows = a->n_rows; P.n_heads = a->n_heads; P.seq_rows = a->seq_rows;
    P.lse = (float *)a->d_workspace;
    P.rowdot = (float *)((char *)a->d_workspace + ws_bytes(a->n_rows, a->n_heads) / 2);
    P.seed_lo = (uint32_t)a->seed; P.seed_hi = (uint32_t)(a->seed >> 32);
    P.off_lo = (uint32_t)a->offset; P.off_hi = (uint32_t)(a->offset >> 32);
    P.d_stream = d_stream;  // given: seed and base come from the device, a->offset is added to the base
    P.keep_thr = (uint32_t)((double)a->dropout_p * 4294967296.0);  // floor(p 2^32), p < 1
    P.keep_scale = 1.0f / (1.0f - a->dropout_p);
    return P;
}
bool drops(const AnceAttn16Args *a) { return a->training != 0 && a->dropout_p > 0.0f; }

template <class X>
void launch_forward(const AnceAttn16Args *args, const AttnParams16 &P, hipStream_t st) {
    const dim3 grid((unsigned)((args->max_seq_len + AH_TILE - 1) / AH_TILE), (unsigned)args->n_heads, (unsigned)args->n_seq);
    const int mode = drop_mode(drops(args), P.d_stream);
    if (mode == DROP_DEVICE) hipLaunchKernelGGL((attn16_fwd_kernel<X, DROP_DEVICE>), grid, dim3(AH_THREADS), 0, st, P);
    else if (mode == DROP_HOST) hipLaunchKernelGGL((attn16_fwd_kernel<X, DROP_HOST>), grid, dim3(AH_THREADS), 0, st, P);
    else hipLaunchKernelGGL((attn16_fwd_kernel<X, DROP_NONE>), grid, dim3(AH_THREADS), 0, st, P);
}
template <class X>
void launch_backward(const AnceAttn16Args *args, const AttnParams16 &P, hipStream_t st) {
    const unsigned tiles = (unsigned)((args->max_seq_len + AH_TILE - 1) / AH_TILE), nh = (unsigned)args->n_heads, ns = (unsigned)args->n_seq;
    hipLaunchKernelGGL((attn16_rowdot_kernel<X>), dim3((unsigned)((args->max_seq_len + 31) / 32), nh, ns), dim3(256), 0, st, P);
    const int mode = drop_mode(drops(args), P.d_stream);
    if (mode == DROP_DEVICE) {
        hipLaunchKernelGGL((attn16_dkv_kernel<X, DROP_DEVICE>), dim3(tiles, nh, ns), dim3(AH_THREADS), 0, st, P);
        hipLaunchKernelGGL((attn16_dq_kernel<X, DROP_DEVICE>), dim3(tiles, nh, ns), dim3(AH_THREADS), 0, st, P);
    } else if (mode == DROP_HOST) {
        hipLaunchKernelGGL((attn16_dkv_kernel<X, DROP_HOST>), dim3(tiles, nh, ns), dim3(AH_THREADS), 0, st, P);
        hipLaunchKernelGGL((attn16_dq_kernel<X, DROP_HOST>), dim3(tiles, nh, ns), dim3(AH_THREADS), 0, st, P);
    } else {
        hipLaunchKernelGGL((attn16_dkv_kernel<X, DROP_NONE>), dim3(tiles, nh, ns), dim3(AH_THREADS), 0, st, P);
        hipLaunchKernelGGL((attn16_dq_kernel<X, DROP_NONE>), dim3(tiles, nh, ns), dim3(AH_THREADS), 0, st, P);
    }
}

}  // namespace
}  // namespace ance

extern "C" size_t ance_attention16_workspace_bytes(int64_t n_rows, int n_heads) {
    using namespace ance;
    return shape_ok(n_rows, n_heads) ? ws_bytes(n_rows, n_heads) : 0;
}

static int ance_attention16_forward_impl(const char *fn, const AnceAttn16Args *args, const uint64_t *d_stream, void *stream) {
    using namespace ance;
    if (!stream_aligned(d_stream)) return refuse(fn, "alignment: d_stream is not 16-byte aligned");
    if (const char *why = check_args(args)) return refuse(fn, why);
    const AttnParams16 P = params(args, d_stream);
    if (args->dtype == ANCE_DTYPE_F16) launch_forward<F16>(args, P, (hipStream_t)stream);
    else launch_forward<BF16>(args, P, (hipStream_t)stream);
    return check_launch(fn);
}

static int ance_attention16_backward_impl(const char *fn, const AnceAttn16Args *args, const AnceAttn16GradArgs *grads,
                                          const uint64_t *d_stream, void *stream) {
    using namespace ance;
    if (!stream_aligned(d_stream)) return refuse(fn, "alignment: d_stream is not 16-byte aligned");
    if (const char *why = check_args(args)) return refuse(fn, why);
    if (!grads) return refuse(fn, "null pointer");
    if (const char *why = check_matrix(grads->dctx, grads->ld_dctx, args->n_heads)) return refuse(fn, why);
    if (const char *why = check_matrix(grads->dq, grads->ld_dq, args->n_heads)) return refuse(fn, why);
    if (const char *why = check_matrix(grads->dk, grads->ld_dk, args->n_heads)) return refuse(fn, why);
    if (const char *why = check_matrix(grads->dv, grads->ld_dv, args->n_heads)) return refuse(fn, why);
    AttnParams16 P = params(args, d_stream);
    P.dctx = grads->dctx; P.dq = grads->dq; P.dk = grads->dk; P.dv = grads->dv;
    P.ld_dctx = grads->ld_dctx; P.ld_dq = grads->ld_dq; P.ld_dk = grads->ld_dk; P.ld_dv = grads->ld_dv;
    if (args->dtype == ANCE_DTYPE_F16) launch_backward<F16>(args, P, (hipStream_t)stream);
    else launch_backward<BF16>(args, P, (hipStream_t)stream);
    return check_launch(fn);
}

// The entry points: each with its sibling that takes the device dropout stream (include/ance_amd.h); the plain one passes none.
extern "C" int ance_attention16_forward(const AnceAttn16Args *args, void *stream) {
    return ance_attention16_forward_impl("ance_attention16_forward", args, nullptr, stream);
}
extern "C" int ance_attention16_forward_dstream(const AnceAttn16Args *args, const uint64_t *d_stream, void *stream) {
    return ance_attention16_forward_impl("ance_attention16_forward_dstream", args, d_stream, stream);
}
extern "C" int ance_attention16_backward(const AnceAttn16Args *args, const AnceAttn16GradArgs *grads, void *stream) {
    return ance_attention16_backward_impl("ance_attention16_backward", args, grads, nullptr, stream);
}
extern "C" int ance_attention16_backward_dstream(const AnceAttn16Args *args, const AnceAttn16GradArgs *grads, const uint64_t *d_stream,
                                                 void *stream) {
    return ance_attention16_backward_impl("ance_attention16_backward_dstream", args, grads, d_stream, stream);
}
