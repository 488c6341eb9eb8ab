// The encoder's small kernels (encoder.hip has the forwards that launch them): conversion, embedding, [CLS] gather, weight
// preparation and head.  The kernels that touch a residual stream are templates of the hidden width H (768 or 1024; head dimension
// 64 at both) and of the stream's storage FORM; what differs between the forms is an `if constexpr` away from what they share.
#pragma once
#include "common.h"
#include "gemm_f16.h"

namespace ance {
namespace {

constexpr int HEAD_OUT = 768;  // embeddingHead output (model/models.py:145), at either width

// ---- the three storage forms of a residual stream -----------------------------------------------
// Rows of a pre-LayerNorm stream with what their consumers need to normalise them (encoder.hip, file header):
//   FORM_F32    fp32 mode: fp32 rows [rows, H] + the (mean, rstd) of every row
//   FORM_PLANES fp16 mode: v = hi + lo, lo = fp16(v - hi), as two planes [rows, H] + the slice partials (gemm_f16.h: PartFormat)
//   FORM_PAIR   split mode: pair rows [rows, 2 H] (common.h: pair_hi_col / pair_lo_col) + the slice partials
enum { FORM_F32 = 0, FORM_PLANES = 1, FORM_PAIR = 2 };
template <int FORM> struct Rows;
template <> struct Rows<FORM_F32> { float *x, *stats; };
template <> struct Rows<FORM_PLANES> { _Float16 *hi, *lo; float *part; };
template <> struct Rows<FORM_PAIR> { _Float16 *xp; float *part; };

__device__ __forceinline__ void split_store(const f32x4 v, _Float16 *hi, _Float16 *lo, int c4) {
    const f16x4 h = cvt_f16x4_pinned(v);
    const f16x4 r = f16x4{(_Float16)(v[0] - (float)h[0]), (_Float16)(v[1] - (float)h[1]), (_Float16)(v[2] - (float)h[2]),
                          (_Float16)(v[3] - (float)h[3])};
    reinterpret_cast<f16x4 *>(hi)[c4] = h;
    reinterpret_cast<f16x4 *>(lo)[c4] = r;
}
__device__ __forceinline__ f32x4 pair_load(const _Float16 *hi, const _Float16 *lo, int c4) {
    const f16x4 h = reinterpret_cast<const f16x4 *>(hi)[c4], r = reinterpret_cast<const f16x4 *>(lo)[c4];
    return f32x4{(float)h[0] + (float)r[0], (float)h[1] + (float)r[1], (float)h[2] + (float)r[2], (float)h[3] + (float)r[3]};
}

// columns 4 c4 .. 4 c4 + 3 of row `row` as fp32
template <int H, int FORM>
__device__ __forceinline__ f32x4 rows_load4(const Rows<FORM> &r, size_t row, int c4) {
    if constexpr (FORM == FORM_F32) return reinterpret_cast<const f32x4 *>(r.x + row * H)[c4];
    else if constexpr (FORM == FORM_PLANES) return pair_load(r.hi + row * H, r.lo + row * H, c4);
    else return pair_load4(r.xp + row * 2 * H, H, c4 * 4);
}
// (mean, rstd) of row `row`: as stored, or recomputed from the slice partials (every lane: 24 cached floats)
template <int H, int FORM>
__device__ __forceinline__ void rows_stats(const Rows<FORM> &r, size_t row, float eps, float *mean, float *rstd) {
    if constexpr (FORM == FORM_F32) { *mean = r.stats[2 * row]; *rstd = r.stats[2 * row + 1]; }
    else stats_from_parts<H>(r.part + row * PART_FLOATS, eps, mean, rstd);
    asm volatile("" : "+v"(*mean));  // consumers subtract the ROUNDED mean: without the barrier hipcc fuses its last product into x - mean
}

__global__ void cvt_f32_f16_kernel(const float *src, _Float16 *dst, size_t n) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) dst[i] = (_Float16)src[i];
}

// ---- embeddings ------------------------------------------------------------------------------------
// slice statistics of an embedding row (PartFormat): lanes 16 j .. 16 j + 15 hold the (mean, M2) of columns 256 k + 64 j .. + 63.
// 768: one slice per 16 lanes; 1024: two adjacent 64-column halves merged into one 128-column slice (part_merge)
template <int H>
__device__ __forceinline__ void store_embed_part(float *part, int t, int k, int l, float m64, float q64) {
    if constexpr (H == 1024) {
        const float mo = __shfl_xor(m64, 16), qo = __shfl_xor(q64, 16);
        if ((l & 31) == 0) {
            float m, q;
            part_merge(m64, q64, mo, qo, &m, &q);
            *reinterpret_cast<float2 *>(part + (size_t)t * PART_FLOATS + (2 * k + (l >> 5)) * 2) = make_float2(m, q);
        }
    } else if ((l & 15) == 0) {
        float *pp = part + ((size_t)t * 12 + 4 * k + (l >> 4)) * 2;  // (12 slices x 2 = PART_FLOATS)
        pp[0] = m64;
        pp[1] = q64;
    }
}

// The split mode stores its embedding rows times EMB_SCALE: the lo half of a pair is unscaled (common.h), i.e. good to 2^-25 ABSOLUTE,
// which is fp32-grade for the O(1) post-residual streams but not for an embedding sum of magnitude 0.05 (trained BERT / RoBERTa
// checkpoints) that a LayerNorm with rstd ~ 20 then blows up.  A LayerNorm is scale-invariant up to its epsilon: the two
// consumers of this stream (layer 0's Q | K | V GEMM and the residual of its attention-output GEMM) run with eps EMB_SCALE^2 -- powers
// of two, so (v s - mean s) and rstd / s are the unscaled values' bits.
constexpr float EMB_SCALE = 16.0f;

// embeddings -> rows of the pre-LayerNorm stream (FORM_PLANES: the (hi, lo) pair; FORM_PAIR: pair rows of the sum times EMB_SCALE,
// range-guarded) + their slice statistics (the format the RESLN epilogues leave: gemm_f16.h, PartFormat); one wave per token, 16 lanes
// per 64 columns
template <int H, int FORM>
__global__ void __launch_bounds__(256) embed_kernel(const int *tok_id, const int *tok_pos, int Tpad, const float *word,
                                                    const float *pos, const float *type0, int vocab, int max_pos,
                                                    const Rows<FORM> out, unsigned *faults) {
    static_assert(FORM == FORM_PLANES || FORM == FORM_PAIR, "the fp32 mode embeds with embed32_kernel");
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int l = threadIdx.x & 63;
    if (t >= Tpad) return;
    int id = tok_id[t], p = tok_pos[t];
    id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
    p = p < 0 ? 0 : (p >= max_pos ? max_pos - 1 : p);
    const f32x4 *w4 = reinterpret_cast<const f32x4 *>(word + (size_t)id * H);
    const f32x4 *p4 = reinterpret_cast<const f32x4 *>(pos + (size_t)p * H);
    const f32x4 *t4 = reinterpret_cast<const f32x4 *>(type0);
    float mx = 0.f;
#pragma unroll
    for (int k = 0; k < H / 256; ++k) {
        const int c4 = k * 64 + l;  // columns 4 c4 .. 4 c4 + 3
        f32x4 v = (w4[c4] + t4[c4]) + p4[c4];  // same association as the reference: (word + type) + pos
        if constexpr (FORM == FORM_PAIR) {
            v = v * EMB_SCALE;
            range_track4(v, &mx);
            pair_store4(v, out.xp + (size_t)t * 2 * H, H, c4 * 4);
        } else {
            split_store(v, out.hi + (size_t)t * H, out.lo + (size_t)t * H, c4);
        }
        const float m64 = row16_sum((v[0] + v[1]) + (v[2] + v[3])) * (1.0f / 64.0f);
        const float d0 = v[0] - m64, d1 = v[1] - m64, d2 = v[2] - m64, d3 = v[3] - m64;
        const float q64 = row16_sum((d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3));
        store_embed_part<H>(out.part, t, k, l, m64, q64);
    }
    if constexpr (FORM == FORM_PAIR) range_report(mx, faults);
}

// last layer, CLS-only tail: compact rows + slice partials of the [CLS] tokens; rows S..S_pad zeroed.  16 bytes per lane and
// step: a pair row whole, or 8 bytes of each plane
template <int H, int FORM>
__global__ void __launch_bounds__(256) gather_cls_kernel(const Rows<FORM> src, const int *seq_off, int S, int S_pad,
                                                         const Rows<FORM> dst) {
    static_assert(FORM == FORM_PLANES || FORM == FORM_PAIR, "the fp32 mode has no CLS-only tail");
    const int s = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int l = threadIdx.x & 63;
    if (s >= S_pad) return;
    const bool real = s < S;
    const size_t row = real ? (size_t)seq_off[s] : 0;
#pragma unroll
    for (int k = 0; k < H / 256; ++k) {
        const int c = k * 64 + l;
        if constexpr (FORM == FORM_PAIR) {
            const f16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
            reinterpret_cast<f16x8 *>(dst.xp + (size_t)s * 2 * H)[c] = real ? reinterpret_cast<const f16x8 *>(src.xp + row * 2 * H)[c] : z;
        } else {
            const f16x4 z = {0, 0, 0, 0};
            reinterpret_cast<f16x4 *>(dst.hi + (size_t)s * H)[c] = real ? reinterpret_cast<const f16x4 *>(src.hi + row * H)[c] : z;
            reinterpret_cast<f16x4 *>(dst.lo + (size_t)s * H)[c] = real ? reinterpret_cast<const f16x4 *>(src.lo + row * H)[c] : z;
        }
    }
    // pad rows: mean 0, variance 1 -- a finite rstd
    if (l < PART_FLOATS)
        dst.part[(size_t)s * PART_FLOATS + l] = real ? src.part[row * PART_FLOATS + l] : ((l & 1) ? (float)PartFormat<H>::COLS : 0.f);
}

// ---- weight preparation ----------------------------------------------------------------------------
// fp16 mode: weight load with the LayerNorm folded in (K = H columns): W16[n][k] = fp16(gamma[k] W[n][k]),
// csum[n] = sum_k W16[n][k] (over the ROUNDED values), bout[n] = b[n] + sum_k beta[k] W[n][k].  One wave per row.
template <int H>
__global__ void __launch_bounds__(256) fold_weight_kernel(const float *W, const float *b, const float *gamma, const float *beta,
                                                          int N, _Float16 *W16, float *csum, float *bout) {
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int l = threadIdx.x & 63;
    if (n >= N) return;
    const f32x4 *w4 = reinterpret_cast<const f32x4 *>(W + (size_t)n * H);
    float cs = 0.f, bs = 0.f;
#pragma unroll
    for (int k = 0; k < H / 256; ++k) {
        const int c4 = k * 64 + l;
        const f32x4 w = w4[c4], g = reinterpret_cast<const f32x4 *>(gamma)[c4], be = reinterpret_cast<const f32x4 *>(beta)[c4];
        const f16x4 h = f16x4{(_Float16)(g[0] * w[0]), (_Float16)(g[1] * w[1]), (_Float16)(g[2] * w[2]), (_Float16)(g[3] * w[3])};
        reinterpret_cast<f16x4 *>(W16 + (size_t)n * H)[c4] = h;
        cs += ((float)h[0] + (float)h[1]) + ((float)h[2] + (float)h[3]);
        bs += (be[0] * w[0] + be[1] * w[1]) + (be[2] * w[2] + be[3] * w[3]);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        cs += __shfl_xor(cs, off);
        bs += __shfl_xor(bs, off);
    }
    if (l == 0) {
        csum[n] = cs;
        bout[n] = b[n] + bs;
    }
}

// Per-matrix scale of the split GEMM's weights: s = 2^p with max |g (.) W| s in [2^13, 2^14).  Pair halves are UNSCALED differences
// (common.h): lo = fp16(w s - hi) of an element below 2^-3 is an fp16 subnormal, good to 2^-25 absolute -- with the largest element
// at 2^13 that is 2^-38 of it, i.e. nothing (unscaled, a 0.02 weight would keep 19 bits).  wabsmax_kernel leaves max |g (.) W| as
// float bits (non-negative floats order as integers) with atomicMax; one slot per weight matrix, Q / K / V share one.
__global__ void __launch_bounds__(256) wabsmax_kernel(const float *W, const float *gamma, int N, int K, unsigned *slot) {
    const size_t total4 = (size_t)N * K / 4;
    float m = 0.f;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total4; i += (size_t)gridDim.x * 256) {
        f32x4 w = reinterpret_cast<const f32x4 *>(W)[i];
        if (gamma) w = w * reinterpret_cast<const f32x4 *>(gamma)[i % (size_t)(K / 4)];
        m = fmaxf(m, fmaxf(fmaxf(fabsf(w[0]), fabsf(w[1])), fmaxf(fabsf(w[2]), fabsf(w[3]))));
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
    if ((threadIdx.x & 63) == 0 && m > 0.f && m < INFINITY) atomicMax(slot, __builtin_bit_cast(unsigned, m));
}
__device__ __forceinline__ float weight_pair_scale(const unsigned *slot) {
    const float m = __builtin_bit_cast(float, *slot);
    if (!(m > 0.f)) return 1.0f;
    int e;
    (void)frexpf(m, &e);  // m in [2^(e-1), 2^e)
    int p = 14 - e;
    p = p < -60 ? -60 : (p > 60 ? 60 : p);
    return ldexpf(1.0f, p);
}

// weight load for the split GEMM: row n of W [N, K] -> pair row (common.h) of  s (g (.) W)  (g = the LayerNorm weight folded in, or
// null; s = the matrix's power-of-two scale, its inverse left in *winv for the GEMM epilogue), csum[n] = sum_k (hi + lo) / s
// (what the MFMAs actually multiply), bout[n] = b[n] + sum_k beta[k] W[n][k].  One wave per row.
__global__ void __launch_bounds__(256) split_weight_kernel(const float *W, const float *b, const float *gamma, const float *beta,
                                                           int N, int K, const unsigned *slot, _Float16 *Wp, float *csum, float *bout,
                                                           float *winv) {
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int l = threadIdx.x & 63;
    if (n >= N) return;
    const float sc = weight_pair_scale(slot);
    if (n == 0 && l == 0) *winv = 1.0f / sc;
    const f32x4 *w4 = reinterpret_cast<const f32x4 *>(W + (size_t)n * K);
    _Float16 *row = Wp + (size_t)n * 2 * K;
    float cs = 0.f, bs = 0.f;
    for (int c4 = l; c4 < K / 4; c4 += 64) {
        f32x4 w = w4[c4];
        if (gamma) {
            const f32x4 g = reinterpret_cast<const f32x4 *>(gamma)[c4], be = reinterpret_cast<const f32x4 *>(beta)[c4];
            bs += (be[0] * w[0] + be[1] * w[1]) + (be[2] * w[2] + be[3] * w[3]);
            w = w * g;
        }
        w = w * sc;
        pair_store4(w, row, K, c4 * 4);
        const f32x4 back = pair_load4(row, K, c4 * 4);
        cs += (back[0] + back[1]) + (back[2] + back[3]);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        cs += __shfl_xor(cs, off);
        bs += __shfl_xor(bs, off);
    }
    if (l == 0) {
        if (csum) csum[n] = cs * (1.0f / sc);
        if (bout) bout[n] = b[n] + bs;
    }
}

// ---- head --------------------------------------------------------------------------------------------
// Both head kernels read the last layer's LayerNorm of the [CLS] rows, recomputed from the pre-LayerNorm stream `pre` (file header of
// encoder.hip); compact: row s already is the [CLS] row of sequence s (CLS-only tail), else it is row seq_off[s].

// Output of a tower without embeddingHead (DPR's BERT): those rows as they are, one block per sequence.
template <int H, int FORM>
__global__ void __launch_bounds__(256) head_kernel(const Rows<FORM> pre, float eps, const float *lng, const float *lnb,
                                                   const int *seq_off, int compact, float *out, unsigned *faults) {
    const int s = blockIdx.x, tid = threadIdx.x;
    const size_t row = (size_t)(compact ? s : seq_off[s]);
    float mean_h, rstd_h;
    rows_stats<H>(pre, row, eps, &mean_h, &rstd_h);
    f32x4 *dst = reinterpret_cast<f32x4 *>(out + (size_t)s * HEAD_OUT);
    for (int c4 = tid; c4 < H / 4; c4 += 256)
        dst[c4] = ln_apply4(rows_load4<H>(pre, row, c4), mean_h, rstd_h, reinterpret_cast<const f32x4 *>(lng)[c4],
                            reinterpret_cast<const f32x4 *>(lnb)[c4]);
    // a NaN anywhere in the row (or an infinity: rstd 0) shows in its statistics: count the row (ance_encoder_range_faults [1])
    if (tid == 0 && faults && (!(fabsf(mean_h) < INFINITY) || !(rstd_h > 0.f && rstd_h < INFINITY))) atomicAdd(faults + 1, 1u);
}

// embeddingHead as one fp32 MFMA GEMM over the [CLS] rows (model/models.py:145-152):
// z[s][n] = sum_k LN(cls_s)[k] W[n][k] + b[n]; 32 sequences x 128 features per workgroup, one 32 x 32 tile per wave
// (v_mfma_f32_32x32x2_f32: exact fp32 products, fp32 accumulation in k order).  The 32 normalised [CLS] rows are staged
// once in LDS (96.5 KiB at H = 768, 128.5 KiB at 1024); W rows stream from L2 as 16-byte pieces per lane.  A block per sequence
// re-read the whole 2.36 MB W (2 GB of L2 reads per 883 rows, 166 us); this reads it 28 times.
template <int H>
constexpr int HEAD_LDA = H + 4;  // floats; 16 lanes x stride 4 banks: conflict-free ds_read_b128
template <int H>
constexpr size_t HEAD_LDS_BYTES = (size_t)32 * HEAD_LDA<H> * sizeof(float);
static_assert(HEAD_LDS_BYTES<1024> <= 160 * 1024, "head GEMM LDS at hidden 1024");

template <int H, int FORM>
__global__ void __launch_bounds__(256) head_gemm_kernel(const Rows<FORM> pre, float eps, const float *lng, const float *lnb,
                                                        const int *seq_off, int compact, int S, const float *W, const float *b,
                                                        float *out) {
    extern __shared__ __attribute__((aligned(16))) float cls[];
    const int s0 = blockIdx.x * 32, n0 = blockIdx.y * 128;
    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, g = l >> 5, i = l & 31;
    // stage LN(pre)[cls] of 32 sequences: wave w takes rows w, w + 4, ...
    for (int r = w; r < 32; r += 4) {
        const int s = s0 + r;
        f32x4 *dst = reinterpret_cast<f32x4 *>(cls + r * HEAD_LDA<H>);
        if (s < S) {
            const size_t row = (size_t)(compact ? s : seq_off[s]);
            float mean, rstd;
            rows_stats<H>(pre, row, eps, &mean, &rstd);
#pragma unroll 1  // (unrolled, the loads of every step are hoisted together: 10 more VGPRs than the MFMA loop needs, a wave less per SIMD)
            for (int k = 0; k < H / 256; ++k) {
                const int c4 = k * 64 + l;
                dst[c4] = ln_apply4(rows_load4<H>(pre, row, c4), mean, rstd, reinterpret_cast<const f32x4 *>(lng)[c4],
                                    reinterpret_cast<const f32x4 *>(lnb)[c4]);
            }
        } else {
#pragma unroll
            for (int k = 0; k < H / 256; ++k) dst[k * 64 + l] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }
    __syncthreads();
    // MFMA rows (A operand) = sequences, columns (B operand) = features n0 + 32 w + i; k-step j of a 16-byte piece uses
    // k = 8 s' + 4 g + j on both sides
    const float *ap = cls + i * HEAD_LDA<H> + 4 * g;
    const float *wp = W + (size_t)(n0 + 32 * w + i) * H + 4 * g;
    f32x16 acc = {0};
#pragma unroll 4
    for (int kk = 0; kk < H / 8; ++kk) {
        const f32x4 a = *reinterpret_cast<const f32x4 *>(ap + kk * 8);
        const f32x4 bb = *reinterpret_cast<const f32x4 *>(wp + kk * 8);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], bb[j], acc, 0, 0, 0);
    }
    // acc[r]: sequence s0 + (r & 3) + 8 (r >> 2) + 4 g, feature n0 + 32 w + i
    const int n = n0 + 32 * w + i;
    const float bias = b[n];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int s = s0 + (r & 3) + 8 * (r >> 2) + 4 * g;
        if (s < S) out[(size_t)s * HEAD_OUT + n] = acc[r] + bias;
    }
}

// final LayerNorm (model/models.py:146,152 "norm") of the head output, in place; one wave per sequence
// (a NaN anywhere upstream of a row -- or an infinity -- shows in these statistics: such rows are counted in faults[1])
__global__ void __launch_bounds__(256) head_ln_kernel(float *out, int S, const float *gamma, const float *beta, unsigned *faults) {
    const int s = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int l = threadIdx.x & 63;
    if (s >= S) return;
    f32x4 *z4 = reinterpret_cast<f32x4 *>(out + (size_t)s * HEAD_OUT);
    f32x4 v[3];
    float sm = 0.f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        v[k] = z4[k * 64 + l];
        sm += (v[k][0] + v[k][1]) + (v[k][2] + v[k][3]);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sm += __shfl_xor(sm, off);
    const float mean = sm * (1.0f / HEAD_OUT);
    float q = 0.f;
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float a = v[k][j] - mean;
            q += a * a;
        }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) q += __shfl_xor(q, off);
    const float rstd = rsqrtf(q * (1.0f / HEAD_OUT) + 1e-5f);
    if (l == 0 && faults && (!(fabsf(mean) < INFINITY) || !(rstd > 0.f && rstd < INFINITY))) atomicAdd(faults + 1, 1u);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int c4 = k * 64 + l;
        z4[c4] = ln_apply4(v[k], mean, rstd, reinterpret_cast<const f32x4 *>(gamma)[c4], reinterpret_cast<const f32x4 *>(beta)[c4]);
    }
}

}  // namespace
}  // namespace ance
