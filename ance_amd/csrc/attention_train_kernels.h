// The kernels of the trainers' self-attention core with its gradient, once, for both precisions of its rows (attention_train.hip:
// X = F32, include/ance_amd.h: ance_attention_forward / _backward; attention_train_half.hip: X = F16 / BF16, ance_attention16_*).
// transformers' eager BertSelfAttention between the three Linear outputs and context_layer, per sequence s (len valid rows, a
// right-padded prefix) and head h of width 64:
//     S = Q K^T * 0.125 over keys j < len;  P = softmax_j(S) (fp32);  P' = keep o P / (1 - p) (training, p > 0), else P;
//     ctx = P' V
//     dV = P'^T dctx;  dP = keep o (dctx V^T) / (1 - p);  dS = P o (dP - D), D_i = sum_j dP_ij P_ij = dctx_i . ctx_i;
//     dQ = 0.125 dS K;  dK = 0.125 dS^T Q
// Pad keys (j >= len) are skipped.  In fp32 that IS the reference's additive -10000 mask: a pad key's term is exp(s - 10000 - max),
// which underflows to exactly 0 for every score an fp32 tower can produce, so neither the row's sum nor ctx sees it.  Pad query
// rows are not computed: in the padded form (seq_rows > 0) the owning workgroups write them as zeros, in the packed form (seq_rows
// = 0) there are none and nothing outside the valid rows is written; a sequence of length 0 is skipped (its rows zeroed likewise).
//
// Every product runs on the matrix cores, 32x32 MFMAs with fp32 accumulation.  A workgroup is two waves; a wave owns 32 rows of the
// tile its workgroup owns and meets the other side in 32-row blocks staged in LDS (rows past len staged as zeros, never read).  All
// three main kernels keep the score block in the MFMA's C/D layout -- lane l: column l & 31, rows 8a + 4(l>>5) + b of register
// 4a + b -- and feed it back as the next product's B operand WITHOUT leaving the registers: a product sums over its k index in any
// order, so the second product takes its k-steps in the order the registers hold them (the policies say how).
//   forward  (q tile 64 x head x seq): S^T = K Q^T (lane = query: max, sum, rescale in-lane + one xor-32 exchange), online
//            softmax over ascending key blocks, ctx^T += V^T P'^T; writes ctx and lse = max + log(sum).  Nothing of size L^2.
//   rowdot   D = dctx . ctx per (head, row) into the workspace.
//   dkv      (key tile 64 x head x seq) owns dK, dV of its keys: walks the query blocks in ascending order; S = Q K^T (lane = key),
//            P = exp(S - lse) recomputed, dP = dctx V^T, dV^T += dctx^T P', dK^T += Q^T dS.
//   dq       (q tile 64 x head x seq) owns dQ of its rows: walks the key blocks; S^T, P^T, dP^T = V dctx^T, dQ^T += K^T dS^T.
// No atomics, one owner per output tile, fixed block order: the same inputs give the same bits.  The grid comes from host values
// only; workgroups exit on the device lengths (clamped to max_seq_len and to n_rows), so nothing waits for the host.
// Dropout: Philox4x32-10, key (seed lo, seed hi), counter (i * 128 + (j >> 2), s * n_heads + h, offset lo, offset hi), word j & 3
// decides key j of query i: keep iff word >= floor(p 2^32).  The forward and dq kernels hold four consecutive keys of one query in a
// lane (one Philox call per four elements); dkv holds one key of sixteen queries, and the four lanes of a quad (four consecutive
// keys) share each query's call: one call per four elements there too, the words exchanged by DPP quad broadcasts.
//
// X is the policy of a precision: the element type T of the rows in memory, and the primitives in which the two cores differ --
// how a 32-row block is staged in LDS and multiplied, whether a C/D block is rounded before it is fed back, where the 0.125 enters,
// which exp is used, how the row-dot splits a row over lanes, and how dkv is scheduled.  Everything else is the kernels' one text.
#pragma once
#include "attention_common.h"

#include <type_traits>

namespace ance {
namespace {

constexpr int AT_THREADS = 128, AT_TILE = 64, AT_BLK = 32;

struct AttnParams {
    const void *q, *k, *v, *ctx, *dctx;  // rows of X::T
    void *ctx_out, *dq, *dk, *dv;
    int64_t ld_q, ld_k, ld_v, ld_ctx, ld_dctx, ld_dq, ld_dk, ld_dv;
    const int32_t *seq_first, *seq_len;
    int max_seq_len, n_rows, n_heads, seq_rows;
    float *lse, *rowdot;  // [n_heads][n_rows] each (workspace)
    uint32_t seed_lo, seed_hi, off_lo, off_hi, keep_thr;
    float keep_scale;
    const uint64_t *d_stream;  // null, or the device stream {seed, base} (philox.h: drop_stream)
};

// What a kernel keeps of a 32-row block in LDS is named by the products that read it: X::Image<ROWS, COLS>::Rows serves the "rows"
// products and ::Cols the "cols" ones -- two LDS variables, each an LdsImage or, where the precision keeps nothing there, NoImage.
template <class E, int N>
struct alignas(16) LdsImage {
    E m[N];
};
struct NoImage {};
// The policies' register carriers (Own, the 16-bit Packed) are plain arrays, a row image and a transposed image are two LDS variables
// and pack_block fills a buffer of the caller's on purpose: wrapped in structs, the same values leave the compiler with other
// register promotions and LDS address arithmetic -- other schedules and register counts (profiles/r19_attention_unify.json compares
// the instruction streams).

// ---- the fp32 policy -------------------------------------------------------------------------------------------------------------
// v_mfma_f32_32x32x2_f32: bitwise an fmaf chain.  The k-step (a, b) of a "cols" product takes key (or query) 8a + b from the lower
// half-wave and 8a + 4 + b from the upper one, which is what register 4a + b of a C/D block holds.  The same freedom lets the
// 64-deep head dimension be split as d = 32 (l>>5) + kk: a lane's own row piece is 32 contiguous floats.  One LDS image of a block,
// [32][68] floats, serves both products.
struct F32 {
    typedef float T;
    typedef f32x4 V4;
    typedef f32x4 Piece;                     // 16 bytes of a row
    static constexpr int PPR_LOG2 = 4;       // 16 pieces per 64-element row
    static constexpr int LD = 68;            // LDS row stride 68 floats: conflict-free ds_read_b128 rows
    static constexpr float PRE = 0.125f, POST = 1.0f;  // forward and dq: Q is scaled as it is loaded (dkv scales S: its own rows are K, V)
    // dkv stages in place under two waves per SIMD: its four accumulators leave no registers to carry the next block across the products
    static constexpr bool DKV_PREFETCH = false;
    static constexpr int DKV_WAVES_PER_EU = 2;

    typedef LdsImage<float, AT_BLK * LD> Rows;
    template <bool ROWS, bool COLS>
    struct Image {  // one image, whatever reads it
        typedef typename F32::Rows Rows;
        typedef NoImage Cols;
    };
    struct Block {  // a fetched block on its way to LDS
        f32x4 v[AT_BLK * 16 / AT_THREADS];
    };
    typedef float Own[32];  // a lane's 32-float piece of its own row (columns 32 (l>>5) ..)
    struct Packed {};  // no buffer: a C/D block is the next product's B operand as it is

    static __device__ __forceinline__ float ex(float x) { return expf(x); }

    // 32 rows x 64 floats from row0 of src (already at the head's columns), in two halves so that the loads of the next block are
    // in flight while this one is multiplied: fetch_block into registers (rows >= valid are zeros, never read), then put_block
    // into LDS one iteration later
    static __device__ __forceinline__ void fetch_block(Block *b, const float *src, int64_t ld, int64_t row0, int valid, int tid) {
#pragma unroll
        for (int t = 0; t < AT_BLK * 16 / AT_THREADS; ++t) {
            const int e = tid + t * AT_THREADS, r = e >> 4, c = (e & 15) * 4;
            b->v[t] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (r < valid) b->v[t] = *reinterpret_cast<const f32x4 *>(src + (row0 + r) * ld + c);
        }
    }
    static __device__ __forceinline__ void put_block(Rows *dst, NoImage *, const Block &b, int tid) {
        float *m = dst->m;  // a pointer, not the member array: the stores below are 16-byte aligned, as their type says
#pragma unroll
        for (int t = 0; t < AT_BLK * 16 / AT_THREADS; ++t) {
            const int e = tid + t * AT_THREADS, r = e >> 4, c = (e & 15) * 4;
            *reinterpret_cast<f32x4 *>(m + r * LD + c) = b.v[t];
        }
    }

    // the lane's own row piece, times scale; zeros for a row that is not valid
    static __device__ __forceinline__ void load_own(Own reg, const float *src, int64_t ld, int64_t row, bool valid, int half, float scale) {
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
            if (valid) v = *reinterpret_cast<const f32x4 *>(src + row * ld + 32 * half + 4 * c);
#pragma unroll
            for (int e = 0; e < 4; ++e) reg[4 * c + e] = v[e] * scale;
        }
    }

    // acc[m][n] += sum_d rows[m = l & 31][d] reg[n = l & 31][d]: the LDS block supplies A, the lane's row piece B
    static __device__ __forceinline__ f32x16 mma_block_rows(const Rows &blk, const Own reg, int lane, f32x16 acc) {
        const float *row = blk.m + (lane & 31) * LD + 32 * (lane >> 5);
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const f32x4 a = *reinterpret_cast<const f32x4 *>(row + 4 * c);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[e], reg[4 * c + e], acc, 0, 0, 0);
        }
        return acc;
    }

    // pack_block(x, buffer): what mma_block_cols takes as b -- here x itself
    static __device__ __forceinline__ f32x16 pack_block(const f32x16 x, Packed) { return x; }

    // acc0[d][n] += sum_r blk[r][d] b[r][n], acc1 the same for d + 32: b is a C/D-layout block (register 4a + b of lane l: row
    // 8a + 4(l>>5) + b, column l & 31), consumed in place as the B operand
    static __device__ __forceinline__ void mma_block_cols(const Rows &blk, const NoImage &, const f32x16 b, int lane, f32x16 *acc0, f32x16 *acc1) {
        const float *col = blk.m + 4 * (lane >> 5) * LD + (lane & 31);
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float *p = col + (8 * a + e) * LD;
                *acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(p[0], b[4 * a + e], *acc0, 0, 0, 0);
                *acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(p[32], b[4 * a + e], *acc1, 0, 0, 0);
            }
    }

    // the row-dot's share of one lane into *d: 16 lanes per (row, head), a piece each
    static __device__ __forceinline__ void piece_dot(const f32x4 &a, const f32x4 &b, float *d) {
        *d = __builtin_fmaf(a[3], b[3], __builtin_fmaf(a[2], b[2], __builtin_fmaf(a[1], b[1], a[0] * b[0])));
    }
};

// ---- the 16-bit policy: T = fp16 or bf16 -------------------------------------------------------------------------------------------
// The arithmetic contract ("rounded" = to nearest even, overflow to +-inf: the plain conversion, v_cvt_f16_f32 /
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
//   Dropout: the Philox counter and keep rule above, unchanged: (seed, offset, s, h, i, j) keeps the same element as in fp32.
//
// Operand maps.  v_mfma_f32_32x32x16_f16 / _bf16: lane l (r = l & 31, h = l >> 5) holds A[r][8h + j] and B[8h + j][r] in element j
// of its 8-element fragment; C/D is that of every 32x32 MFMA: column l & 31, rows 8a + 4h + b in register 4a + b.
//   "rows" product  acc[m][n] = sum_d blk[m][d] own[n][d]  (S, S^T, dP, dP^T): k-step t is d = 16t + 8h + j.  A = 16 bytes of row m
//     of the block's ROW image in LDS ([32][72] T: 144-byte rows), B = 16 bytes of the lane's own row, loaded once from memory.
//   "cols" product  acc[d][n] += sum_r blk[r][d] X[r][n]  with X a C/D-layout block left in its registers (P', dS): registers
//     8s .. 8s + 7 converted to T ARE the B fragment of k-step s, which permutes k inside the step: element j of half h is block row
//     16s + 8(j >> 2) + 4h + (j & 3).  The A fragment follows that order: elements 0..3 = blkT[d][16s + 4h ..], 4..7 =
//     blkT[d][16s + 8 + 4h ..]: two 8-byte reads of the block's TRANSPOSED image ([64][36] T: 72-byte rows, conflict-free), which
//     the staging threads write as (row 2u, row 2u + 1) pairs, one 4-byte store per column.
// A kernel keeps of each block only the images its products read.
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
__device__ __forceinline__ f32x16 mfma16(f16x8 a, f16x8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }
__device__ __forceinline__ f32x16 mfma16(bf16x8 a, bf16x8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }

template <class E>
struct Half16 {
    typedef E T;
    typedef E V8 __attribute__((ext_vector_type(8)));
    typedef E V4 __attribute__((ext_vector_type(4)));
    typedef E V2 __attribute__((ext_vector_type(2)));
    typedef V8 Piece;                   // 16 bytes of a row
    static constexpr int PPR_LOG2 = 3;  // 8 pieces per 64-element row
    static constexpr int LDR = 72;      // row image [32][72]: 144-byte rows, 16-byte aligned
    static constexpr int LDT = 36;      // transposed image [64][36]: 72-byte rows, 8-byte aligned; 18 banks a row: 32 rows x 2 banks, all distinct
    static constexpr float PRE = 1.0f, POST = 0.125f;  // S is scaled in fp32, in every kernel
    static constexpr float LOG2E = 1.4426950408889634f;
    static constexpr bool DKV_PREFETCH = true;     // the next block's loads travel while this block is multiplied, as in the other kernels
    static constexpr int DKV_WAVES_PER_EU = 0;     // no floor

    typedef LdsImage<E, AT_BLK * LDR> Rows;
    typedef LdsImage<E, 64 * LDT> Cols;
    template <bool ROWS, bool COLS>
    struct Image {  // a row image, a transposed image, or both
        typedef std::conditional_t<ROWS, typename Half16::Rows, NoImage> Rows;
        typedef std::conditional_t<COLS, typename Half16::Cols, NoImage> Cols;
    };
    // thread (u = tid >> 3, ch = tid & 7) carries the 16-byte chunk ch of rows 2u and 2u + 1
    struct Block {
        V8 a, b;
    };
    typedef V8 Own[4];  // the lane's own row as the B fragments of the four k-steps: [t] = row[16t + 8 half .. + 7]
    typedef V8 Packed[2];  // a C/D-layout fp32 block, rounded to T, as the two B fragments of the next product

    static __device__ __forceinline__ V8 zero8() { return __builtin_bit_cast(V8, i32x4{0, 0, 0, 0}); }

    // the one exp of this precision: the forward and both backward kernels
    static __device__ __forceinline__ float ex(float x) { return __builtin_amdgcn_exp2f(x * LOG2E); }

    // 32 rows x 64 elements from row0 of src (already at the head's columns); rows >= valid are zeros, never read from memory
    static __device__ __forceinline__ void fetch_block(Block *st, const T *src, int64_t ld, int64_t row0, int valid, int tid) {
        const int u = tid >> 3, ch = tid & 7;
        st->a = zero8();
        st->b = zero8();
        if (2 * u < valid) st->a = *reinterpret_cast<const V8 *>(src + (row0 + 2 * u) * ld + 8 * ch);
        if (2 * u + 1 < valid) st->b = *reinterpret_cast<const V8 *>(src + (row0 + 2 * u + 1) * ld + 8 * ch);
    }
    template <class R, class C>
    static __device__ __forceinline__ void put_block(R *dst, C *dstT, const Block &st, int tid) {
        const int u = tid >> 3, ch = tid & 7;
        if constexpr (std::is_same<R, Rows>::value) {  // through a pointer, not the member array: the stores are aligned as their type says
            T *rows = dst->m;
            *reinterpret_cast<V8 *>(rows + (2 * u) * LDR + 8 * ch) = st.a;
            *reinterpret_cast<V8 *>(rows + (2 * u + 1) * LDR + 8 * ch) = st.b;
        }
        if constexpr (std::is_same<C, Cols>::value) {  // cols[d][r] = block[r][d]
            T *cols = dstT->m;
#pragma unroll
            for (int e = 0; e < 8; ++e) *reinterpret_cast<V2 *>(cols + (8 * ch + e) * LDT + 2 * u) = V2{st.a[e], st.b[e]};
        }
    }

    // the lane's own row; zeros for a row that is not valid.  No pre-scale: S is scaled in fp32
    static __device__ __forceinline__ void load_own(Own reg, const T *src, int64_t ld, int64_t row, bool valid, int half, float) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            reg[t] = zero8();
            if (valid) reg[t] = *reinterpret_cast<const V8 *>(src + row * ld + 16 * t + 8 * half);
        }
    }

    // acc[m][n] += sum_d blk[m = l & 31][d] reg[n = l & 31][d]: the row image supplies A, the lane's own row B
    static __device__ __forceinline__ f32x16 mma_block_rows(const Rows &blk, const Own reg, int lane, f32x16 acc) {
        const T *row = blk.m + (lane & 31) * LDR + 8 * (lane >> 5);
#pragma unroll
        for (int t = 0; t < 4; ++t) acc = mfma16(*reinterpret_cast<const V8 *>(row + 16 * t), reg[t], acc);
        return acc;
    }

    // x rounded to T into the caller's buffer, which is returned: k = the block's row index, permuted inside a step
    static __device__ __forceinline__ const Packed &pack_block(const f32x16 x, Packed &out) {
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int j = 0; j < 8; ++j) out[s][j] = (T)x[8 * s + j];
        return out;
    }

    // acc0[d][n] += sum_r blkT[d][r] b[r][n], acc1 the same for d + 32: A from the transposed image in the k order of pack_block
    template <class R>
    static __device__ __forceinline__ void mma_block_cols(const R &, const Cols &blk, const Packed &b, int lane, f32x16 *acc0, f32x16 *acc1) {
        const T *col = blk.m + (lane & 31) * LDT + 4 * (lane >> 5);
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const V4 lo0 = *reinterpret_cast<const V4 *>(col + 16 * s);
            const V4 hi0 = *reinterpret_cast<const V4 *>(col + 16 * s + 8);
            const V4 lo1 = *reinterpret_cast<const V4 *>(col + 32 * LDT + 16 * s);
            const V4 hi1 = *reinterpret_cast<const V4 *>(col + 32 * LDT + 16 * s + 8);
            *acc0 = mfma16(__builtin_shufflevector(lo0, hi0, 0, 1, 2, 3, 4, 5, 6, 7), b[s], *acc0);
            *acc1 = mfma16(__builtin_shufflevector(lo1, hi1, 0, 1, 2, 3, 4, 5, 6, 7), b[s], *acc1);
        }
    }

    // the row-dot's share of one lane, in fp32, onto *d (0 on entry): 8 lanes per (row, head), a piece each, an ascending fmaf chain
    static __device__ __forceinline__ void piece_dot(const V8 &a, const V8 &b, float *d) {
#pragma unroll
        for (int e = 0; e < 8; ++e) *d = __builtin_fmaf((float)a[e], (float)b[e], *d);
    }
};
typedef Half16<_Float16> F16;
typedef Half16<__bf16> BF16;

// ---- what every precision shares ---------------------------------------------------------------------------------------------------

// word c of the four words that lane E of this lane's quad holds (DPP quad broadcast, then a select on the lane's own c)
template <int E>
__device__ __forceinline__ uint32_t quad_word(const uint32_t w[4], int c) {
    const uint32_t t0 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)w[0], E * 0x55, 0xf, 0xf, false);
    const uint32_t t1 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)w[1], E * 0x55, 0xf, 0xf, false);
    const uint32_t t2 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)w[2], E * 0x55, 0xf, 0xf, false);
    const uint32_t t3 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)w[3], E * 0x55, 0xf, 0xf, false);
    return (c & 2) ? ((c & 1) ? t3 : t2) : ((c & 1) ? t1 : t0);
}

// The padded form (seq_rows > 0): a sequence owns seq_rows rows from its first one, and the rows behind its length are written as
// zeros by the workgroup that owns their tile -- also by one that has nothing else to do.  Rows [max(t0, len), min(t0 + 64, own))
// of the head's 64 columns of dst, own = seq_rows clamped to n_rows - first; nothing when the first row is outside [0, n_rows).
template <class X>
__device__ __forceinline__ void zero_pad_rows(const AttnParams &P, typename X::T *dst, int64_t ld, int first, int len, int t0, int tid) {
    constexpr int PPR = 1 << X::PPR_LOG2;
    if (P.seq_rows <= 0 || first < 0 || first >= P.n_rows) return;
    const int own = P.seq_rows < P.n_rows - first ? P.seq_rows : P.n_rows - first;
    const int lo = t0 > len ? t0 : len, hi = t0 + AT_TILE < own ? t0 + AT_TILE : own;
    for (int e = tid; e < (hi - lo) * PPR; e += AT_THREADS)
        *reinterpret_cast<i32x4 *>(dst + ((int64_t)first + lo + (e >> X::PPR_LOG2)) * ld + (e & (PPR - 1)) * (64 / PPR)) = i32x4{0, 0, 0, 0};  // a 16-byte piece
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
__global__ void __launch_bounds__(AT_THREADS) attn_fwd_kernel(const AttnParams P) {
    typedef typename X::T T;
    typedef typename X::template Image<true, false> KI;  // K feeds S^T
    typedef typename X::template Image<false, true> VI;  // V feeds ctx^T
    __shared__ typename KI::Rows Ks;
    __shared__ typename KI::Cols Kt;
    __shared__ typename VI::Rows Vs;
    __shared__ typename VI::Cols Vt;
    const int s = blockIdx.z, head = blockIdx.y, q0 = blockIdx.x * AT_TILE;
    const DropStream D = drop_stream<DROP>(P);
    int first;
    const int len = seq_bounds(P, s, &first);
    zero_pad_rows<X>(P, (T *)P.ctx_out + 64 * head, P.ld_ctx, first, len, q0, threadIdx.x);
    if (q0 >= len) return;
    const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5;
    const int qi = q0 + 32 * (tid >> 6) + (lane & 31);
    const bool qok = qi < len;
    const int64_t qrow = (int64_t)first + qi;
    typename X::Own qreg;
    X::load_own(qreg, (const T *)P.q + 64 * head, P.ld_q, qrow, qok, half, X::PRE);
    const T *kbase = (const T *)P.k + 64 * head, *vbase = (const T *)P.v + 64 * head;
    f32x16 acc0 = {}, acc1 = {};
    float m = -INFINITY, l = 0.f;
    typename X::Block kn, vn;
    X::fetch_block(&kn, kbase, P.ld_k, (int64_t)first, len, tid);
    X::fetch_block(&vn, vbase, P.ld_v, (int64_t)first, len, tid);
    for (int jb = 0; jb < len; jb += AT_BLK) {
        __syncthreads();
        X::put_block(&Ks, &Kt, kn, tid);
        X::put_block(&Vs, &Vt, vn, tid);
        __syncthreads();
        if (jb + AT_BLK < len) {  // the next block's loads travel while this block is multiplied
            X::fetch_block(&kn, kbase, P.ld_k, (int64_t)first + jb + AT_BLK, len - jb - AT_BLK, tid);
            X::fetch_block(&vn, vbase, P.ld_v, (int64_t)first + jb + AT_BLK, len - jb - AT_BLK, tid);
        }
        f32x16 sc = {};
        sc = X::mma_block_rows(Ks, qreg, lane, sc);  // S^T: rows = keys, column = this lane's query
        float mb = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int j = jb + 8 * (r >> 2) + 4 * half + (r & 3);
            sc[r] = j < len ? sc[r] * X::POST : -INFINITY;
            mb = fmaxf(mb, sc[r]);
        }
        mb = fmaxf(mb, __shfl_xor(mb, 32));
        const float mn = fmaxf(m, mb);  // finite: key 0 is valid and sits in the first block
        const float alpha = X::ex(m - mn);
        float sum = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            sc[r] = X::ex(sc[r] - mn);
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
        typename X::Packed pbuf;
        const auto &pb = X::pack_block(sc, pbuf);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            acc0[r] *= alpha;
            acc1[r] *= alpha;
        }
        X::mma_block_cols(Vs, Vt, pb, lane, &acc0, &acc1);  // ctx^T: rows = d, column = this lane's query
    }
    if (qok) {
        const float inv = (DROP ? P.keep_scale : 1.0f) / l;
        store_row_t<X>((T *)P.ctx_out + qrow * P.ld_ctx + 64 * head, acc0, acc1, half, inv);
        if (half == 0) P.lse[(int64_t)head * P.n_rows + qrow] = m + logf(l);
    }
}

// D[head][row] = dctx[row] . ctx[row] over the head's 64 columns in fp32: a piece per lane (X::piece_dot), fixed xor tree over the
// row's lanes
template <class X>
__global__ void __launch_bounds__(256) attn_rowdot_kernel(const AttnParams P) {
    typedef typename X::T T;
    constexpr int PPR = 1 << X::PPR_LOG2, RPB = 256 / PPR;  // pieces per row, rows per block
    const int s = blockIdx.z, head = blockIdx.y;
    int first;
    const int len = seq_bounds(P, s, &first);
    const int i = blockIdx.x * RPB + (threadIdx.x >> X::PPR_LOG2), c = (threadIdx.x & (PPR - 1)) * (64 / PPR);
    if (blockIdx.x * RPB >= len) return;
    const bool ok = i < len;
    const int64_t row = (int64_t)first + i;
    float d = 0.f;
    if (ok) {
        const typename X::Piece a = *reinterpret_cast<const typename X::Piece *>((const T *)P.dctx + row * P.ld_dctx + 64 * head + c);
        const typename X::Piece b = *reinterpret_cast<const typename X::Piece *>((const T *)P.ctx + row * P.ld_ctx + 64 * head + c);
        X::piece_dot(a, b, &d);
    }
#pragma unroll
    for (int off = PPR / 2; off > 0; off >>= 1) d += __shfl_xor(d, off);
    if (ok && c == 0) P.rowdot[(int64_t)head * P.n_rows + row] = d;
}

template <class X, int DROP>
__global__ void __launch_bounds__(AT_THREADS) attn_dq_kernel(const AttnParams P) {
    typedef typename X::T T;
    typedef typename X::template Image<true, true> KI;   // K feeds S^T and dQ^T
    typedef typename X::template Image<true, false> VI;  // V feeds dP^T
    __shared__ typename KI::Rows Ks;
    __shared__ typename KI::Cols Kt;
    __shared__ typename VI::Rows Vs;
    __shared__ typename VI::Cols Vt;
    const int s = blockIdx.z, head = blockIdx.y, q0 = blockIdx.x * AT_TILE;
    const DropStream D = drop_stream<DROP>(P);
    int first;
    const int len = seq_bounds(P, s, &first);
    zero_pad_rows<X>(P, (T *)P.dq + 64 * head, P.ld_dq, first, len, q0, threadIdx.x);
    if (q0 >= len) return;
    const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5;
    const int qi = q0 + 32 * (tid >> 6) + (lane & 31);
    const bool qok = qi < len;
    const int64_t qrow = (int64_t)first + qi;
    typename X::Own qreg, greg;
    X::load_own(qreg, (const T *)P.q + 64 * head, P.ld_q, qrow, qok, half, X::PRE);
    X::load_own(greg, (const T *)P.dctx + 64 * head, P.ld_dctx, qrow, qok, half, 1.0f);
    const float lse = qok ? P.lse[(int64_t)head * P.n_rows + qrow] : 0.f;
    const float rd = qok ? P.rowdot[(int64_t)head * P.n_rows + qrow] : 0.f;
    const T *kbase = (const T *)P.k + 64 * head, *vbase = (const T *)P.v + 64 * head;
    f32x16 acc0 = {}, acc1 = {};
    typename X::Block kn, vn;
    X::fetch_block(&kn, kbase, P.ld_k, (int64_t)first, len, tid);
    X::fetch_block(&vn, vbase, P.ld_v, (int64_t)first, len, tid);
    for (int jb = 0; jb < len; jb += AT_BLK) {
        __syncthreads();
        X::put_block(&Ks, &Kt, kn, tid);
        X::put_block(&Vs, &Vt, vn, tid);
        __syncthreads();
        if (jb + AT_BLK < len) {  // the next block's loads travel while this block is multiplied
            X::fetch_block(&kn, kbase, P.ld_k, (int64_t)first + jb + AT_BLK, len - jb - AT_BLK, tid);
            X::fetch_block(&vn, vbase, P.ld_v, (int64_t)first + jb + AT_BLK, len - jb - AT_BLK, tid);
        }
        f32x16 sc = {}, dp = {};
        sc = X::mma_block_rows(Ks, qreg, lane, sc);  // S^T
        dp = X::mma_block_rows(Vs, greg, lane, dp);  // dP^T = V dctx^T
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
            const float p = (j < len && qok) ? X::ex(sc[r] * X::POST - lse) : 0.f;
            float g = dp[r];
            if (DROP) g = w[r] >= P.keep_thr ? g * P.keep_scale : 0.f;
            sc[r] = p * (g - rd);  // dS^T
        }
        typename X::Packed dbuf;
        const auto &db = X::pack_block(sc, dbuf);
        X::mma_block_cols(Ks, Kt, db, lane, &acc0, &acc1);  // dQ^T += K^T dS^T
    }
    if (qok) store_row_t<X>((T *)P.dq + qrow * P.ld_dq + 64 * head, acc0, acc1, half, 0.125f);
}

template <class X, int DROP>
__global__ void __launch_bounds__(AT_THREADS, X::DKV_WAVES_PER_EU) attn_dkv_kernel(const AttnParams P) {
    typedef typename X::T T;
    typedef typename X::template Image<true, true> I;  // Q feeds S and dK^T, dctx feeds dP and dV^T
    __shared__ typename I::Rows Qs, Gs;
    __shared__ typename I::Cols Qt, Gt;
    __shared__ __attribute__((aligned(16))) float lse_s[AT_BLK], rd_s[AT_BLK];
    const int s = blockIdx.z, head = blockIdx.y, k0 = blockIdx.x * AT_TILE;
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
    typename X::Own kreg, vreg;  // unscaled in every precision: S is scaled below
    X::load_own(kreg, (const T *)P.k + 64 * head, P.ld_k, krow, kok, half, 1.0f);
    X::load_own(vreg, (const T *)P.v + 64 * head, P.ld_v, krow, kok, half, 1.0f);
    const T *qbase = (const T *)P.q + 64 * head, *gbase = (const T *)P.dctx + 64 * head;
    f32x16 ak0 = {}, ak1 = {}, av0 = {}, av1 = {};
    typename X::Block qn, gn;
    if (X::DKV_PREFETCH) {
        X::fetch_block(&qn, qbase, P.ld_q, (int64_t)first, len, tid);
        X::fetch_block(&gn, gbase, P.ld_dctx, (int64_t)first, len, tid);
    }
    for (int ib = 0; ib < len; ib += AT_BLK) {
        __syncthreads();
        if (!X::DKV_PREFETCH) {  // staged in place (X::DKV_PREFETCH says why)
            X::fetch_block(&qn, qbase, P.ld_q, (int64_t)first + ib, len - ib, tid);
            X::fetch_block(&gn, gbase, P.ld_dctx, (int64_t)first + ib, len - ib, tid);
        }
        X::put_block(&Qs, &Qt, qn, tid);
        X::put_block(&Gs, &Gt, gn, tid);
        if (tid < AT_BLK) {
            const bool ok = ib + tid < len;
            const int64_t o = (int64_t)head * P.n_rows + first + ib + tid;
            lse_s[tid] = ok ? P.lse[o] : 0.f;
            rd_s[tid] = ok ? P.rowdot[o] : 0.f;
        }
        __syncthreads();
        if (X::DKV_PREFETCH && ib + AT_BLK < len) {  // the next block's loads travel while this block is multiplied
            X::fetch_block(&qn, qbase, P.ld_q, (int64_t)first + ib + AT_BLK, len - ib - AT_BLK, tid);
            X::fetch_block(&gn, gbase, P.ld_dctx, (int64_t)first + ib + AT_BLK, len - ib - AT_BLK, tid);
        }
        f32x16 sc = {}, dp = {};
        sc = X::mma_block_rows(Qs, kreg, lane, sc);  // S: rows = queries, column = this lane's key
        dp = X::mma_block_rows(Gs, vreg, lane, dp);  // dP = dctx V^T
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
                const float p = (i < len && kok) ? X::ex(sc[r] * 0.125f - ls[e]) : 0.f;
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
        typename X::Packed pbuf, dbuf;
        const auto &pb = X::pack_block(pd, pbuf);
        const auto &db = X::pack_block(sc, dbuf);
        X::mma_block_cols(Gs, Gt, pb, lane, &av0, &av1);  // dV^T += dctx^T P'
        X::mma_block_cols(Qs, Qt, db, lane, &ak0, &ak1);  // dK^T += Q^T dS
    }
    if (kok) {
        store_row_t<X>((T *)P.dk + krow * P.ld_dk + 64 * head, ak0, ak1, half, 0.125f);
        store_row_t<X>((T *)P.dv + krow * P.ld_dv + 64 * head, av0, av1, half, 1.0f);
    }
}

// ---- the host side of both full cores ------------------------------------------------------------------------------------------------
size_t core_ws_bytes(int64_t n_rows, int n_heads) { return 2 * align_up(sizeof(float) * (size_t)n_rows * (size_t)n_heads, 256); }
size_t core_workspace_query(int64_t n_rows, int n_heads) { return shape_ok(n_rows, 0x7fffffff, n_heads) ? core_ws_bytes(n_rows, n_heads) : 0; }

// An entry point of a full core that accepts `dtypes`: attention_call with the workspace as lse, then D
template <class Launch>
int core_call(const char *fn, unsigned dtypes, const AnceAttn16Args *args, bool backward, const AnceAttn16GradArgs *grads,
              const uint64_t *d_stream, Launch launch) {
    const AttnRules rules = {dtypes, "dtype not ANCE_DTYPE_F16 or ANCE_DTYPE_BF16", args ? core_ws_bytes(args->n_rows, args->n_heads) : 0};
    return attention_call<AttnParams>(fn, rules, args, backward, grads, d_stream, [&](AttnParams P) {
        P.ctx_out = args->ctx;
        P.lse = (float *)args->d_workspace;
        P.rowdot = (float *)((char *)args->d_workspace + rules.ws_bytes / 2);
        launch(P);
    });
}

// One launch forward, three backward: the grid from host values only, the instantiation from how the call draws its masks
template <class X>
void launch_forward(const AnceAttn16Args *args, const AttnParams &P, hipStream_t st) {
    const dim3 grid((unsigned)((args->max_seq_len + AT_TILE - 1) / AT_TILE), (unsigned)args->n_heads, (unsigned)args->n_seq);
    const int mode = drop_mode(drops(args), P.d_stream);
    if (mode == DROP_DEVICE) hipLaunchKernelGGL((attn_fwd_kernel<X, DROP_DEVICE>), grid, dim3(AT_THREADS), 0, st, P);
    else if (mode == DROP_HOST) hipLaunchKernelGGL((attn_fwd_kernel<X, DROP_HOST>), grid, dim3(AT_THREADS), 0, st, P);
    else hipLaunchKernelGGL((attn_fwd_kernel<X, DROP_NONE>), grid, dim3(AT_THREADS), 0, st, P);
}
template <class X>
void launch_backward(const AnceAttn16Args *args, const AttnParams &P, hipStream_t st) {
    constexpr int RPB = 256 >> X::PPR_LOG2;  // the row-dot's rows per block
    const unsigned tiles = (unsigned)((args->max_seq_len + AT_TILE - 1) / AT_TILE), nh = (unsigned)args->n_heads, ns = (unsigned)args->n_seq;
    hipLaunchKernelGGL((attn_rowdot_kernel<X>), dim3((unsigned)((args->max_seq_len + RPB - 1) / RPB), nh, ns), dim3(256), 0, st, P);
    const int mode = drop_mode(drops(args), P.d_stream);
    if (mode == DROP_DEVICE) {
        hipLaunchKernelGGL((attn_dkv_kernel<X, DROP_DEVICE>), dim3(tiles, nh, ns), dim3(AT_THREADS), 0, st, P);
        hipLaunchKernelGGL((attn_dq_kernel<X, DROP_DEVICE>), dim3(tiles, nh, ns), dim3(AT_THREADS), 0, st, P);
    } else if (mode == DROP_HOST) {
        hipLaunchKernelGGL((attn_dkv_kernel<X, DROP_HOST>), dim3(tiles, nh, ns), dim3(AT_THREADS), 0, st, P);
        hipLaunchKernelGGL((attn_dq_kernel<X, DROP_HOST>), dim3(tiles, nh, ns), dim3(AT_THREADS), 0, st, P);
    } else {
        hipLaunchKernelGGL((attn_dkv_kernel<X, DROP_NONE>), dim3(tiles, nh, ns), dim3(AT_THREADS), 0, st, P);
        hipLaunchKernelGGL((attn_dq_kernel<X, DROP_NONE>), dim3(tiles, nh, ns), dim3(AT_THREADS), 0, st, P);
    }
}

}  // namespace
}  // namespace ance
