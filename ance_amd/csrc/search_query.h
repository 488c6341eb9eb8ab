// Per-call query preparation of the two-precision search (ip_topk_fast.hip, step 2) and the error bound of its approximate
// score: the mean query of the call and its per-row share of every score, the fp16 rounding of the queries, 2 eps.
// Included by ip_topk_fast.hip only, into its anonymous namespace.
//
// Error bound.  The image holds xh = fp16(x') with x' = fl32(x - mu), mu = the shard's mean row: q . x = q . (x - mu) + q . mu,
// and the second term is the same for every row of a query, so ranking by q . x' is ranking by q . x -- but |x'| is what the
// fp16 rounding error scales with.  Embeddings of one encoder share a large common component (random-init roberta-base:
// cosine 0.99 between any two passages, scores 737 +- 1.7): without the centring 2 eps is wider than the whole score
// distribution and every query overflows.  The queries get the same treatment: q = mq + dq with mq the mean query of the
// call, q . x' = mq . x' + dq . x'; the first term is a per-ROW constant b (one fp32 pass over the shard per call, the
// accumulators of a corpus tile start from it), and only dq meets the fp16 rounding.  With C the canonical fp32 chain score:
//   rounding dq and x' to fp16, normal range:  |dq . x' - dqh . xh| <= (2^-11 + 2^-11 + 2^-22) |dq| |x'|
//   fp32 accumulation inside / between MFMAs, starting from b:  <= 1.1 d 2^-24 (|dq| + |mq|) |x'|
//   b = fl32 chain of mq . x':                 <= d 2^-24 |mq| |x'|
//   x' = fl32(x - mu), dq = fl32(q - mq):      <= 2^-23 |q| |x'|
//   fp16 subnormal inputs, 2^-25 per element:  <= 2^-25 sqrt(d) (|dq| + |x'|)
//   the chain itself, C vs q . x:              <= d 2^-24 |q| |x|       (the un-centred norms)
// |s~ - (C - q . mu)| <= eps = 1.25 * [ (2^-10 + 1.1 d 2^-24) |dq| X' + 2.1 d 2^-24 |mq| X' + 2^-23 |q| X' + 2^-24 sqrt(d) (|dq| + X') + d 2^-24 |q| X ]
// with X' = max |x'|, X = max |x| (tests/test_eps_bound.py attacks it on the CPU).  tests/test_gpu_search_adversarial.py runs
// the device code on corpora whose true neighbours the filter under-estimates by 30-35 % of 2 eps: a slack about three
// times too small at any site that applies it loses rows there.  The query mean is only used when it
// is a sizeable part of the queries (|mq| > 0.05 X); otherwise mq = 0, dq = q, b = 0 and the bias pass is skipped.
#pragma once
#include "search_image.h"

namespace ance {
namespace {

// the mean query of a call: used only when it is a sizeable part of the queries (|mq| > 0.05 max|x|); decided on the device
struct QueryStat {
    float mq_norm;  // |mq| (0 when not used)
    int use_bias;   // != 0: dq = q - mq goes through the MFMAs, b = mq . x' is added per row
    int bad_image;  // != 0: the image's stamp does not match this call: no kernel touches it, every chunk is redone exactly
};
// searches that found their image stamped for another matrix (or never built) and answered every chunk with the exact scan:
// correct results, several times slower -- counted so that a caller can notice (ance_search_bad_image_calls)
__device__ unsigned long long g_bad_image_calls = 0ull;

__global__ void __launch_bounds__(256) query_mean_decide_kernel(float *mq, int d, const DedupHeader *H, QueryStat *qs, int64_t n,
                                                                const float *x) {
    __shared__ float red[4];
    float s = 0.f;
    for (int c = threadIdx.x; c < d; c += 256) s += mq[c] * mq[c];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    const float nrm = sqrtf(red[0] + red[1] + red[2] + red[3]) * 1.0001f;
    const float xo = __builtin_bit_cast(float, H->xmax_orig_bits);
    const bool bad = H->magic != DEDUP_MAGIC || H->d != (unsigned int)d || H->n != (unsigned long long)n ||
                     H->x_ptr != (unsigned long long)(uintptr_t)x;
    const bool use = !bad && nrm == nrm && nrm < 3.0e38f && xo < 3.0e38f && nrm > 0.05f * xo;
    __syncthreads();
    if (!use)
        for (int c = threadIdx.x; c < d; c += 256) mq[c] = 0.0f;
    if (threadIdx.x == 0) {
        qs->mq_norm = use ? nrm : 0.0f;
        qs->use_bias = use ? 1 : 0;
        qs->bad_image = bad ? 1 : 0;
        if (bad) atomicAdd(&g_bad_image_calls, 1ull);
    }
}

// b[r] = mq . x'(image row r), x' = fl32(x - mu) recomputed from the fp32 shard row: one wave per image row
__global__ void __launch_bounds__(256) row_bias_kernel(const float *x, int d, const DedupHeader *H, const uint32_t *live2row, const float *mu,
                                                       const float *mq, const QueryStat *qs, float *bias) {
    if (!qs->use_bias) return;
    const int l = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t n_live = H->n_live;
    for (int64_t r = (int64_t)blockIdx.x * 4 + w; r < n_live; r += (int64_t)gridDim.x * 4) {
        const float *s = x + (size_t)live2row[r] * d;
        float acc = 0.f;
        for (int k = l * 4; k < d; k += 256) {
            const f32x4 v = *reinterpret_cast<const f32x4 *>(s + k), m4 = *reinterpret_cast<const f32x4 *>(mu + k),
                        q4 = *reinterpret_cast<const f32x4 *>(mq + k);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc = fmaf(q4[e], v[e] - m4[e], acc);
        }
        acc = wave_sum(acc);
        if (l == 0) bias[r] = acc;
    }
}

// fp16(q - mq) + the norms of dq = q - mq and of q for the query chunk: one wave per row
__global__ void __launch_bounds__(256) round_rows_kernel(const float *src, int64_t rows, int d, const float *mq, _Float16 *dst,
                                                         float *norm_c, float *norm_o) {
    const int l = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int64_t row = (int64_t)blockIdx.x * 4 + w; row < rows; row += (int64_t)gridDim.x * 4) {
        float nc, no;
        center_round_row(src + (size_t)row * d, mq, d, l, dst + (size_t)row * d, &nc, &no);
        if (l == 0) {  // NaN stays NaN: the filter's trust test is false for it
            norm_c[row] = nc;
            norm_o[row] = no;
        }
    }
}

// 2 eps of one query (top of this file); INFINITY when fp16 cannot be trusted (a norm above 65504, or not finite)
struct EpsConst {
    float rel_c, acc_m, cen, abs_c, chain_o;  // 1.25 x: (2^-10 + 1.1 d 2^-24), 2.1 d 2^-24, 2^-23, 2^-24 sqrt(d), d 2^-24
};
EpsConst make_eps(int d) {
    EpsConst eps;
    eps.rel_c = 1.25f * (9.765625e-4f + 1.1f * d * 5.9604645e-8f);
    eps.acc_m = 1.25f * 2.1f * d * 5.9604645e-8f;
    eps.cen = 1.25f * 1.1920929e-7f;
    eps.abs_c = 1.25f * 5.9604645e-8f * sqrtf((float)d);
    eps.chain_o = 1.25f * d * 5.9604645e-8f;
    return eps;
}
// qc = |q - mq|, qo = |q|
__device__ __forceinline__ float two_eps(const EpsConst &E, float qc, float qo, const QueryStat *qs, const DedupHeader *H) {
    const float xc = __builtin_bit_cast(float, H->xmax_bits), xo = __builtin_bit_cast(float, H->xmax_orig_bits);
    const bool ok = qc <= 65504.0f && qo < 3.0e38f && xc <= 65504.0f && xo < 3.0e38f;  // false for NaN too
    return ok ? 2.0f * (E.rel_c * qc * xc + E.acc_m * qs->mq_norm * xc + E.cen * qo * xc + E.abs_c * (qc + xc) + E.chain_o * qo * xo)
              : INFINITY;
}

}  // namespace
}  // namespace ance
