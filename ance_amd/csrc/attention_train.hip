// The trainers' self-attention core with its gradient (include/ance_amd.h: ance_attention_forward / ance_attention_backward):
// transformers' eager BertSelfAttention between the three Linear outputs and context_layer, per sequence s (len valid rows, a
// right-padded prefix) and head h of width 64:
//     S = Q K^T * 0.125 over keys j < len;  P = softmax_j(S) (fp32, expf);  P' = keep o P / (1 - p) (training, p > 0), else P;
//     ctx = P' V
//     dV = P'^T dctx;  dP = keep o (dctx V^T) / (1 - p);  dS = P o (dP - D), D_i = sum_j dP_ij P_ij = dctx_i . ctx_i;
//     dQ = 0.125 dS K;  dK = 0.125 dS^T Q
// Pad keys (j >= len) are skipped.  In fp32 that IS the reference's additive -10000 mask: a pad key's term is exp(s - 10000 - max),
// which underflows to exactly 0 for every score an fp32 tower can produce, so neither the row's sum nor ctx sees it.  Pad query
// rows are not computed: in the padded form (seq_rows > 0) the owning workgroups write them as zeros, in the packed form (seq_rows
// = 0) there are none and nothing outside the valid rows is written; a sequence of length 0 is skipped (its rows zeroed likewise).
//
// Every product runs on the fp32 matrix cores (v_mfma_f32_32x32x2_f32: bitwise an fmaf chain).  A workgroup is two waves; a wave owns
// 32 rows of the tile its workgroup owns and meets the other side in 32-row blocks staged in LDS (rows past len staged as zeros,
// never read).  All three main kernels keep the score block in the MFMA's C/D layout -- lane l: column l & 31, rows 8a + 4(l>>5) + b
// of register 4a + b -- and feed it back as the next product's B operand WITHOUT leaving the registers: a product sums over its
// k index in any order, so the k-step (a, b) of the second product takes key (or query) 8a + b from the lower half-wave and
// 8a + 4 + b from the upper one, which is what register 4a + b holds.  The same freedom lets the 64-deep head dimension be
// split as d = 32 (l>>5) + kk: a lane's Q row piece is 32 contiguous floats.
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
#include "common.h"
#include "philox.h"
#include "attention_train.h"

namespace ance {
namespace {

constexpr int AT_THREADS = 128, AT_TILE = 64, AT_BLK = 32, AT_LD = 68;  // LDS row stride 68 floats: conflict-free ds_read_b128 rows

struct AttnParams {
    const float *q, *k, *v, *ctx, *dctx;
    float *ctx_out, *dq, *dk, *dv;
    int64_t ld_q, ld_k, ld_v, ld_ctx, ld_dctx, ld_dq, ld_dk, ld_dv;
    const int32_t *seq_first, *seq_len;
    int max_seq_len, n_rows, n_heads, seq_rows;
    float *lse, *rowdot;  // [n_heads][n_rows] each (workspace)
    uint32_t seed_lo, seed_hi, off_lo, off_hi, keep_thr;
    float keep_scale;
    const uint64_t *d_stream;  // null, or the device stream {seed, base} (philox.h: drop_stream)
};

// quad_word and seq_bounds: attention_train.h (shared with the 16-bit core)

// The padded form (seq_rows > 0): a sequence owns seq_rows rows from its first one, and the rows behind its length are written as
// zeros by the workgroup that owns their tile -- also by one that has nothing else to do.  Rows [max(t0, len), min(t0 + 64, own))
// of the head's 64 columns of dst, own = seq_rows clamped to n_rows - first; nothing when the first row is outside [0, n_rows).
__device__ __forceinline__ void zero_pad_rows(const AttnParams &P, float *dst, int64_t ld, int first, int len, int t0, int tid) {
    if (P.seq_rows <= 0 || first < 0 || first >= P.n_rows) return;
    const int own = P.seq_rows < P.n_rows - first ? P.seq_rows : P.n_rows - first;
    const int lo = t0 > len ? t0 : len, hi = t0 + AT_TILE < own ? t0 + AT_TILE : own;
    for (int e = tid; e < (hi - lo) * 16; e += AT_THREADS)
        *reinterpret_cast<f32x4 *>(dst + ((int64_t)first + lo + (e >> 4)) * ld + (e & 15) * 4) = f32x4{0.f, 0.f, 0.f, 0.f};
}

// 32 rows x 64 floats from row0 of src (already at the head's columns) into dst [32][AT_LD], in two halves so that the loads of the
// next block are in flight while this one is multiplied: fetch_block into registers (rows >= valid are zeros, never read), then
// put_block into LDS one iteration later
struct BlockRegs {
    f32x4 v[AT_BLK * 16 / AT_THREADS];
};
__device__ __forceinline__ void fetch_block(BlockRegs *b, const float *src, int64_t ld, int64_t row0, int valid, int tid) {
#pragma unroll
    for (int t = 0; t < AT_BLK * 16 / AT_THREADS; ++t) {
        const int e = tid + t * AT_THREADS, r = e >> 4, c = (e & 15) * 4;
        b->v[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (r < valid) b->v[t] = *reinterpret_cast<const f32x4 *>(src + (row0 + r) * ld + c);
    }
}
__device__ __forceinline__ void put_block(float *dst, const BlockRegs &b, int tid) {
#pragma unroll
    for (int t = 0; t < AT_BLK * 16 / AT_THREADS; ++t) {
        const int e = tid + t * AT_THREADS, r = e >> 4, c = (e & 15) * 4;
        *reinterpret_cast<f32x4 *>(dst + r * AT_LD + c) = b.v[t];
    }
}

// a lane's 32-float piece of its own row (columns 32 (l>>5) ..), times scale; zeros for a row that is not valid
__device__ __forceinline__ void load_row_piece(float reg[32], const float *src, int64_t ld, int64_t row, bool valid, int half, float scale) {
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
        if (valid) v = *reinterpret_cast<const f32x4 *>(src + row * ld + 32 * half + 4 * c);
#pragma unroll
        for (int e = 0; e < 4; ++e) reg[4 * c + e] = v[e] * scale;
    }
}

// acc[m][n] += sum_d rows[m = l & 31][d] reg[n = l & 31][d]: the LDS block supplies A, the lane's row piece B
__device__ __forceinline__ f32x16 mma_block_rows(const float *blk, const float reg[32], int lane, f32x16 acc) {
    const float *row = blk + (lane & 31) * AT_LD + 32 * (lane >> 5);
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const f32x4 a = *reinterpret_cast<const f32x4 *>(row + 4 * c);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[e], reg[4 * c + e], acc, 0, 0, 0);
    }
    return acc;
}

// acc0[d][n] += sum_r blk[r][d] b[r][n], acc1 the same for d + 32: b is a C/D-layout block (register 4a + b of lane l: row
// 8a + 4(l>>5) + b, column l & 31), consumed in place as the B operand
__device__ __forceinline__ void mma_block_cols(const float *blk, const f32x16 b, int lane, f32x16 *acc0, f32x16 *acc1) {
    const float *col = blk + 4 * (lane >> 5) * AT_LD + (lane & 31);
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float *p = col + (8 * a + e) * AT_LD;
            *acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(p[0], b[4 * a + e], *acc0, 0, 0, 0);
            *acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(p[32], b[4 * a + e], *acc1, 0, 0, 0);
        }
}

// a C/D-layout accumulator pair (rows = head columns d, column = the lane's own row) -> 64 floats of the lane's row, times scale
__device__ __forceinline__ void store_row_t(float *dst, const f32x16 acc0, const f32x16 acc1, int half, float scale) {
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        *reinterpret_cast<f32x4 *>(dst + 8 * a + 4 * half) =
            f32x4{acc0[4 * a] * scale, acc0[4 * a + 1] * scale, acc0[4 * a + 2] * scale, acc0[4 * a + 3] * scale};
        *reinterpret_cast<f32x4 *>(dst + 32 + 8 * a + 4 * half) =
            f32x4{acc1[4 * a] * scale, acc1[4 * a + 1] * scale, acc1[4 * a + 2] * scale, acc1[4 * a + 3] * scale};
    }
}

template <int DROP>
__global__ void __launch_bounds__(AT_THREADS) attn_fwd_kernel(const AttnParams P) {
    __shared__ __attribute__((aligned(16))) float Ks[AT_BLK * AT_LD], Vs[AT_BLK * AT_LD];
    const int s = blockIdx.z, head = blockIdx.y, q0 = blockIdx.x * AT_TILE;
    const DropStream D = drop_stream<DROP>(P);
    int first;
    const int len = seq_bounds(P, s, &first);
    zero_pad_rows(P, P.ctx_out + 64 * head, P.ld_ctx, first, len, q0, threadIdx.x);
    if (q0 >= len) return;
    const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5;
    const int qi = q0 + 32 * (tid >> 6) + (lane & 31);
    const bool qok = qi < len;
    const int64_t qrow = (int64_t)first + qi;
    float qreg[32];
    load_row_piece(qreg, P.q + 64 * head, P.ld_q, qrow, qok, half, 0.125f);
    const float *kbase = P.k + 64 * head, *vbase = P.v + 64 * head;
    f32x16 acc0 = {}, acc1 = {};
    float m = -INFINITY, l = 0.f;
    BlockRegs kn, vn;
    fetch_block(&kn, kbase, P.ld_k, (int64_t)first, len, tid);
    fetch_block(&vn, vbase, P.ld_v, (int64_t)first, len, tid);
    for (int jb = 0; jb < len; jb += AT_BLK) {
        __syncthreads();
        put_block(Ks, kn, tid);
        put_block(Vs, vn, tid);
        __syncthreads();
        if (jb + AT_BLK < len) {  // the next block's loads travel while this block is multiplied
            fetch_block(&kn, kbase, P.ld_k, (int64_t)first + jb + AT_BLK, len - jb - AT_BLK, tid);
            fetch_block(&vn, vbase, P.ld_v, (int64_t)first + jb + AT_BLK, len - jb - AT_BLK, tid);
        }
        f32x16 sc = {};
        sc = mma_block_rows(Ks, qreg, lane, sc);  // S^T: rows = keys, column = this lane's query
        float mb = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int j = jb + 8 * (r >> 2) + 4 * half + (r & 3);
            sc[r] = j < len ? sc[r] : -INFINITY;
            mb = fmaxf(mb, sc[r]);
        }
        mb = fmaxf(mb, __shfl_xor(mb, 32));
        const float mn = fmaxf(m, mb);  // finite: key 0 is valid and sits in the first block
        const float alpha = expf(m - mn);
        float sum = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            sc[r] = expf(sc[r] - mn);
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
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            acc0[r] *= alpha;
            acc1[r] *= alpha;
        }
        mma_block_cols(Vs, sc, lane, &acc0, &acc1);  // ctx^T: rows = d, column = this lane's query
    }
    if (qok) {
        const float inv = (DROP ? P.keep_scale : 1.0f) / l;
        store_row_t(P.ctx_out + qrow * P.ld_ctx + 64 * head, acc0, acc1, half, inv);
        if (half == 0) P.lse[(int64_t)head * P.n_rows + qrow] = m + logf(l);
    }
}

// D[head][row] = dctx[row] . ctx[row] over the head's 64 columns: 16 lanes per (row, head), fixed xor tree
__global__ void __launch_bounds__(256) attn_rowdot_kernel(const AttnParams P) {
    const int s = blockIdx.z, head = blockIdx.y;
    int first;
    const int len = seq_bounds(P, s, &first);
    const int i = blockIdx.x * 16 + (threadIdx.x >> 4), c = (threadIdx.x & 15) * 4;
    if (blockIdx.x * 16 >= len) return;
    const bool ok = i < len;
    const int64_t row = (int64_t)first + i;
    float d = 0.f;
    if (ok) {
        const f32x4 a = *reinterpret_cast<const f32x4 *>(P.dctx + row * P.ld_dctx + 64 * head + c);
        const f32x4 b = *reinterpret_cast<const f32x4 *>(P.ctx + row * P.ld_ctx + 64 * head + c);
        d = __builtin_fmaf(a[3], b[3], __builtin_fmaf(a[2], b[2], __builtin_fmaf(a[1], b[1], a[0] * b[0])));
    }
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) d += __shfl_xor(d, off);
    if (ok && c == 0) P.rowdot[(int64_t)head * P.n_rows + row] = d;
}

template <int DROP>
__global__ void __launch_bounds__(AT_THREADS) attn_dq_kernel(const AttnParams P) {
    __shared__ __attribute__((aligned(16))) float Ks[AT_BLK * AT_LD], Vs[AT_BLK * AT_LD];
    const int s = blockIdx.z, head = blockIdx.y, q0 = blockIdx.x * AT_TILE;
    const DropStream D = drop_stream<DROP>(P);
    int first;
    const int len = seq_bounds(P, s, &first);
    zero_pad_rows(P, P.dq + 64 * head, P.ld_dq, first, len, q0, threadIdx.x);
    if (q0 >= len) return;
    const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5;
    const int qi = q0 + 32 * (tid >> 6) + (lane & 31);
    const bool qok = qi < len;
    const int64_t qrow = (int64_t)first + qi;
    float qreg[32], greg[32];
    load_row_piece(qreg, P.q + 64 * head, P.ld_q, qrow, qok, half, 0.125f);
    load_row_piece(greg, P.dctx + 64 * head, P.ld_dctx, qrow, qok, half, 1.0f);
    const float lse = qok ? P.lse[(int64_t)head * P.n_rows + qrow] : 0.f;
    const float rd = qok ? P.rowdot[(int64_t)head * P.n_rows + qrow] : 0.f;
    const float *kbase = P.k + 64 * head, *vbase = P.v + 64 * head;
    f32x16 acc0 = {}, acc1 = {};
    BlockRegs kn, vn;
    fetch_block(&kn, kbase, P.ld_k, (int64_t)first, len, tid);
    fetch_block(&vn, vbase, P.ld_v, (int64_t)first, len, tid);
    for (int jb = 0; jb < len; jb += AT_BLK) {
        __syncthreads();
        put_block(Ks, kn, tid);
        put_block(Vs, vn, tid);
        __syncthreads();
        if (jb + AT_BLK < len) {  // the next block's loads travel while this block is multiplied
            fetch_block(&kn, kbase, P.ld_k, (int64_t)first + jb + AT_BLK, len - jb - AT_BLK, tid);
            fetch_block(&vn, vbase, P.ld_v, (int64_t)first + jb + AT_BLK, len - jb - AT_BLK, tid);
        }
        f32x16 sc = {}, dp = {};
        sc = mma_block_rows(Ks, qreg, lane, sc);  // S^T
        dp = mma_block_rows(Vs, greg, lane, dp);  // dP^T = V dctx^T
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
            const float p = (j < len && qok) ? expf(sc[r] - lse) : 0.f;
            float g = dp[r];
            if (DROP) g = w[r] >= P.keep_thr ? g * P.keep_scale : 0.f;
            sc[r] = p * (g - rd);  // dS^T
        }
        mma_block_cols(Ks, sc, lane, &acc0, &acc1);  // dQ^T += K^T dS^T
    }
    if (qok) store_row_t(P.dq + qrow * P.ld_dq + 64 * head, acc0, acc1, half, 0.125f);
}

template <int DROP>
__global__ void __launch_bounds__(AT_THREADS, 2) attn_dkv_kernel(const AttnParams P) {
    __shared__ __attribute__((aligned(16))) float Qs[AT_BLK * AT_LD], Gs[AT_BLK * AT_LD];
    __shared__ __attribute__((aligned(16))) float lse_s[AT_BLK], rd_s[AT_BLK];
    const int s = blockIdx.z, head = blockIdx.y, k0 = blockIdx.x * AT_TILE;
    const DropStream D = drop_stream<DROP>(P);
    int first;
    const int len = seq_bounds(P, s, &first);
    zero_pad_rows(P, P.dk + 64 * head, P.ld_dk, first, len, k0, threadIdx.x);
    zero_pad_rows(P, P.dv + 64 * head, P.ld_dv, first, len, k0, threadIdx.x);
    if (k0 >= len) return;
    const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5;
    const int kj = k0 + 32 * (tid >> 6) + (lane & 31);
    const bool kok = kj < len;
    const int64_t krow = (int64_t)first + kj;
    float kreg[32], vreg[32];
    load_row_piece(kreg, P.k + 64 * head, P.ld_k, krow, kok, half, 1.0f);
    load_row_piece(vreg, P.v + 64 * head, P.ld_v, krow, kok, half, 1.0f);
    const float *qbase = P.q + 64 * head, *gbase = P.dctx + 64 * head;
    f32x16 ak0 = {}, ak1 = {}, av0 = {}, av1 = {};
    for (int ib = 0; ib < len; ib += AT_BLK) {
        __syncthreads();
        {   // staged in place: this kernel's four accumulators leave no registers to carry the next block across the products
            BlockRegs qn, gn;
            fetch_block(&qn, qbase, P.ld_q, (int64_t)first + ib, len - ib, tid);
            fetch_block(&gn, gbase, P.ld_dctx, (int64_t)first + ib, len - ib, tid);
            put_block(Qs, qn, tid);
            put_block(Gs, gn, tid);
        }
        if (tid < AT_BLK) {
            const bool ok = ib + tid < len;
            const int64_t o = (int64_t)head * P.n_rows + first + ib + tid;
            lse_s[tid] = ok ? P.lse[o] : 0.f;
            rd_s[tid] = ok ? P.rowdot[o] : 0.f;
        }
        __syncthreads();
        f32x16 sc = {}, dp = {};
        sc = mma_block_rows(Qs, kreg, lane, sc);  // S: rows = queries, column = this lane's key
        dp = mma_block_rows(Gs, vreg, lane, dp);  // dP = dctx V^T
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
                const float p = (i < len && kok) ? expf(sc[r] * 0.125f - ls[e]) : 0.f;
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
        mma_block_cols(Gs, pd, lane, &av0, &av1);  // dV^T += dctx^T P'
        mma_block_cols(Qs, sc, lane, &ak0, &ak1);  // dK^T += Q^T dS
    }
    if (kok) {
        store_row_t(P.dk + krow * P.ld_dk + 64 * head, ak0, ak1, half, 0.125f);
        store_row_t(P.dv + krow * P.ld_dv + 64 * head, av0, av1, half, 1.0f);
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
    if (ld % 4 != 0 || ld < 64 * n_heads) return "stride: not a multiple of 4 or below 64 * n_heads";
    return nullptr;
}
const char *check_args(const AnceAttnTrainArgs *a) {
    if (!a) return "null pointer";
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
AttnParams params(const AnceAttnTrainArgs *a, const uint64_t *d_stream) {
    AttnParams P = {};
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
bool drops(const AnceAttnTrainArgs *a) { return a->training != 0 && a->dropout_p > 0.0f; }

}  // namespace
}  // namespace ance

extern "C" size_t ance_attention_workspace_bytes(int64_t n_rows, int n_heads) {
    using namespace ance;
    return shape_ok(n_rows, n_heads) ? ws_bytes(n_rows, n_heads) : 0;
}

static int ance_attention_forward_impl(const char *fn, const AnceAttnTrainArgs *args, const uint64_t *d_stream, void *stream) {
    using namespace ance;
    if (!stream_aligned(d_stream)) return refuse(fn, "alignment: d_stream is not 16-byte aligned");
    if (const char *why = check_args(args)) return refuse(fn, why);
    const AttnParams P = params(args, d_stream);
    const dim3 grid((unsigned)((args->max_seq_len + AT_TILE - 1) / AT_TILE), (unsigned)args->n_heads, (unsigned)args->n_seq);
    hipStream_t st = (hipStream_t)stream;
    const int mode = drop_mode(drops(args), d_stream);
    if (mode == DROP_DEVICE) hipLaunchKernelGGL(attn_fwd_kernel<DROP_DEVICE>, grid, dim3(AT_THREADS), 0, st, P);
    else if (mode == DROP_HOST) hipLaunchKernelGGL(attn_fwd_kernel<DROP_HOST>, grid, dim3(AT_THREADS), 0, st, P);
    else hipLaunchKernelGGL(attn_fwd_kernel<DROP_NONE>, grid, dim3(AT_THREADS), 0, st, P);
    return check_launch(fn);
}

static int ance_attention_backward_impl(const char *fn, const AnceAttnTrainArgs *args, const AnceAttnGradArgs *grads,
                                        const uint64_t *d_stream, void *stream) {
    using namespace ance;
    if (!stream_aligned(d_stream)) return refuse(fn, "alignment: d_stream is not 16-byte aligned");
    if (const char *why = check_args(args)) return refuse(fn, why);
    if (!grads) return refuse(fn, "null pointer");
    if (const char *why = check_matrix(grads->dctx, grads->ld_dctx, args->n_heads)) return refuse(fn, why);
    if (const char *why = check_matrix(grads->dq, grads->ld_dq, args->n_heads)) return refuse(fn, why);
    if (const char *why = check_matrix(grads->dk, grads->ld_dk, args->n_heads)) return refuse(fn, why);
    if (const char *why = check_matrix(grads->dv, grads->ld_dv, args->n_heads)) return refuse(fn, why);
    AttnParams P = params(args, d_stream);
    P.dctx = grads->dctx; P.dq = grads->dq; P.dk = grads->dk; P.dv = grads->dv;
    P.ld_dctx = grads->ld_dctx; P.ld_dq = grads->ld_dq; P.ld_dk = grads->ld_dk; P.ld_dv = grads->ld_dv;
    const unsigned tiles = (unsigned)((args->max_seq_len + AT_TILE - 1) / AT_TILE), nh = (unsigned)args->n_heads, ns = (unsigned)args->n_seq;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(attn_rowdot_kernel, dim3((unsigned)((args->max_seq_len + 15) / 16), nh, ns), dim3(256), 0, st, P);
    const int mode = drop_mode(drops(args), d_stream);
    if (mode == DROP_DEVICE) {
        hipLaunchKernelGGL(attn_dkv_kernel<DROP_DEVICE>, dim3(tiles, nh, ns), dim3(AT_THREADS), 0, st, P);
        hipLaunchKernelGGL(attn_dq_kernel<DROP_DEVICE>, dim3(tiles, nh, ns), dim3(AT_THREADS), 0, st, P);
    } else if (mode == DROP_HOST) {
        hipLaunchKernelGGL(attn_dkv_kernel<DROP_HOST>, dim3(tiles, nh, ns), dim3(AT_THREADS), 0, st, P);
        hipLaunchKernelGGL(attn_dq_kernel<DROP_HOST>, dim3(tiles, nh, ns), dim3(AT_THREADS), 0, st, P);
    } else {
        hipLaunchKernelGGL(attn_dkv_kernel<DROP_NONE>, dim3(tiles, nh, ns), dim3(AT_THREADS), 0, st, P);
        hipLaunchKernelGGL(attn_dq_kernel<DROP_NONE>, dim3(tiles, nh, ns), dim3(AT_THREADS), 0, st, P);
    }
    return check_launch(fn);
}

// The entry points: each with its sibling that takes the device dropout stream (include/ance_amd.h); the plain one passes none.
extern "C" int ance_attention_forward(const AnceAttnTrainArgs *args, void *stream) {
    return ance_attention_forward_impl("ance_attention_forward", args, nullptr, stream);
}
extern "C" int ance_attention_forward_dstream(const AnceAttnTrainArgs *args, const uint64_t *d_stream, void *stream) {
    return ance_attention_forward_impl("ance_attention_forward_dstream", args, d_stream, stream);
}
extern "C" int ance_attention_backward(const AnceAttnTrainArgs *args, const AnceAttnGradArgs *grads, void *stream) {
    return ance_attention_backward_impl("ance_attention_backward", args, grads, nullptr, stream);
}
extern "C" int ance_attention_backward_dstream(const AnceAttnTrainArgs *args, const AnceAttnGradArgs *grads, const uint64_t *d_stream,
                                               void *stream) {
    return ance_attention_backward_impl("ance_attention_backward_dstream", args, grads, d_stream, stream);
}
