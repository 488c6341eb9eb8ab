// The DPR trainer's default objective, in-batch negatives (drivers/run_ann_dpr.py:356-365, also its evaluate_dev), with its gradient:
//     scores = q ctx^T [nq, nc];  loss = mean_i -log_softmax(scores[i])[positive_idx[i]];
//     n_correct = #{i : argmax_j scores[i][j] == positive_idx[i]}   (the lowest j among equal scores)
//     gS = (softmax(scores) - onehot) grad_output / nq;  gq = gS ctx;  gctx = gS^T q
// Forward, three launches: scores (fp32 FMA GEMM) -> one workgroup per row (max / argmax, log-sum-exp, the row's loss) -> one
// workgroup that sums the rows.  Backward, three launches: gS -> gq -> gctx.  The sizes are tiny (at most 1024 x 2048 x 1024: 2.1
// GFMA per product), so the three products share one plain LDS-tiled fp32 kernel: 64 x 64 outputs per workgroup, 4 x 4 per thread,
// every output an fmaf chain over 16-deep k tiles in ascending k, the tiles' sums added in fp64 in ascending order and rounded
// once (a softmax over scores in the hundreds sees what 64 fp32 additions at that magnitude lose).  No atomics, no
// split-k: the same inputs give the same bits.  HBM traffic: forward reads (nq + nc) d 4 bytes and writes nq nc 4 (the scores stay
// in the caller's workspace for the backward); backward reads the scores and writes gS once (8 nq nc bytes), reads gS twice and
// q, ctx once each, writes (nq + nc) d 4.  grad_output is a device scalar: nothing waits for the host.
// A positive_idx outside [0, nc) is never used as an address: the row's loss is NaN (so is the mean), the row never counts as
// correct, it is counted in d_counts[1], and the backward makes that row of gS NaN.
#include "common.h"

namespace ance {
namespace {

constexpr int TM = 64, TN = 64, TK = 16, GEMM_THREADS = 256;

// C [M, N] = A B^T over k.  AK: A is stored [M][K] (k contiguous), else [K][M].  BK: B is stored [N][K], else [K][N].
template <bool AK, bool BK>
__global__ void __launch_bounds__(GEMM_THREADS) gemm_f32_kernel(const float *A, const float *B, float *C, int M, int N, int K) {
    __shared__ float As[TK][TM + 1], Bs[TK][TN + 1];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int m0 = blockIdx.y * TM, n0 = blockIdx.x * TN;
    double acc[4][4] = {};  // the tiles' sums: scores of LayerNorm rows reach 900, where 64 fp32 additions cost 1e-4 -- a softmax sees that
    for (int k0 = 0; k0 < K; k0 += TK) {
#pragma unroll
        for (int t = 0; t < TM * TK / GEMM_THREADS; ++t) {
            const int e = tid + t * GEMM_THREADS;
            {
                const int m = AK ? e / TK : e % TM, k = AK ? e % TK : e / TM;
                const int gm = m0 + m, gk = k0 + k;
                As[k][m] = (gm < M && gk < K) ? (AK ? A[(int64_t)gm * K + gk] : A[(int64_t)gk * M + gm]) : 0.f;
            }
            {
                const int n = BK ? e / TK : e % TN, k = BK ? e % TK : e / TN;
                const int gn = n0 + n, gk = k0 + k;
                Bs[k][n] = (gn < N && gk < K) ? (BK ? B[(int64_t)gn * K + gk] : B[(int64_t)gk * N + gn]) : 0.f;
            }
        }
        __syncthreads();
        float part[4][4] = {};
#pragma unroll
        for (int k = 0; k < TK; ++k) {
            float av[4], bv[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) { av[i] = As[k][ty * 4 + i]; bv[i] = Bs[k][tx * 4 + i]; }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) part[i][j] = __builtin_fmaf(av[i], bv[j], part[i][j]);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] += (double)part[i][j];
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int gm = m0 + ty * 4 + i;
        if (gm >= M) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int gn = n0 + tx * 4 + j;
            if (gn < N) C[(int64_t)gm * N + gn] = (float)acc[i][j];
        }
    }
}

template <bool AK, bool BK>
void launch_gemm(const float *A, const float *B, float *C, int M, int N, int K, hipStream_t st) {
    hipLaunchKernelGGL((gemm_f32_kernel<AK, BK>), dim3((unsigned)((N + TN - 1) / TN), (unsigned)((M + TM - 1) / TM)), dim3(GEMM_THREADS), 0,
                       st, A, B, C, M, N, K);
}

// one workgroup per row: (max, lowest argmax) and sum of exp in a fixed order (thread-strided, xor-shuffle tree, the four waves in order)
// The log-sum-exp is kept as its two terms, the row's max and log(sum exp(s - max)): at scores in the hundreds (LayerNorm outputs of
// 768 / 1024 columns) their sum is only known to ulp(|s|), 6e-5 at 900, and exp(s - (max + log sum)) would carry that as a RELATIVE
// error into every gradient; (s - max) is exact for the leading scores and the small term is subtracted from it at full precision.
__global__ void __launch_bounds__(256) inbatch_rows_kernel(const float *S, const int64_t *pos, int nc, float *row_max, float *log_sum,
                                                           float *loss_rows, int32_t *flags) {
    __shared__ float s_v[4];
    __shared__ int s_i[4];
    const int i = blockIdx.x, tid = threadIdx.x;
    const float *row = S + (int64_t)i * nc;
    float mx = -INFINITY;
    int arg = 0x7fffffff;
    for (int j = tid; j < nc; j += 256) {
        const float v = row[j];
        if (v > mx) { mx = v; arg = j; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_xor(mx, off);
        const int oi = __shfl_xor(arg, off);
        if (ov > mx || (ov == mx && oi < arg)) { mx = ov; arg = oi; }
    }
    if ((tid & 63) == 0) { s_v[tid >> 6] = mx; s_i[tid >> 6] = arg; }
    __syncthreads();
    mx = s_v[0];
    arg = s_i[0];
#pragma unroll
    for (int w = 1; w < 4; ++w)
        if (s_v[w] > mx || (s_v[w] == mx && s_i[w] < arg)) { mx = s_v[w]; arg = s_i[w]; }
    __syncthreads();
    float sum = 0.f;
    for (int j = tid; j < nc; j += 256) sum += expf(row[j] - mx);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
    if ((tid & 63) == 0) s_v[tid >> 6] = sum;
    __syncthreads();
    if (tid == 0) {
        const float l = logf(((s_v[0] + s_v[1]) + s_v[2]) + s_v[3]);
        const int64_t p = pos[i];
        const bool ok = p >= 0 && p < (int64_t)nc;
        row_max[i] = mx;
        log_sum[i] = l;
        loss_rows[i] = ok ? (mx - row[p]) + l : __builtin_nanf("");
        flags[i] = ok ? (arg == (int)p ? 1 : 0) : 2;  // bit 0: correct, bit 1: index out of range
    }
}

// mean of the rows' losses and the two counts, one workgroup, fixed order
__global__ void __launch_bounds__(1024) inbatch_reduce_kernel(const float *loss_rows, const int32_t *flags, int nq, float *loss_mean,
                                                              int64_t *counts) {
    __shared__ float s[1024];
    __shared__ int c1[1024], c2[1024];
    const int tid = threadIdx.x;
    float acc = 0.f;
    int a1 = 0, a2 = 0;
    for (int i = tid; i < nq; i += 1024) {
        acc += loss_rows[i];
        a1 += flags[i] & 1;
        a2 += flags[i] >> 1;
    }
    s[tid] = acc; c1[tid] = a1; c2[tid] = a2;
    __syncthreads();
    for (int off = 512; off > 0; off >>= 1) {
        if (tid < off) { s[tid] += s[tid + off]; c1[tid] += c1[tid + off]; c2[tid] += c2[tid + off]; }
        __syncthreads();
    }
    if (tid == 0) {
        loss_mean[0] = s[0] / (float)nq;
        counts[0] = c1[0];
        counts[1] = c2[0];
    }
}

__global__ void __launch_bounds__(256) inbatch_gs_kernel(const float *S, const float *row_max, const float *log_sum, const int64_t *pos,
                                                         int nq, int nc, const float *grad_output, float *gS) {
    const int i = blockIdx.x;
    const float s = grad_output[0] / (float)nq, mx = row_max[i], l = log_sum[i];
    const int64_t p = pos[i];
    const bool ok = p >= 0 && p < (int64_t)nc;
    for (int j = threadIdx.x; j < nc; j += 256) {
        const int64_t o = (int64_t)i * nc + j;
        const float sm = expf((S[o] - mx) - l);
        gS[o] = ok ? (sm - ((int64_t)j == p ? 1.0f : 0.0f)) * s : __builtin_nanf("");
    }
}

struct Layout {
    size_t off_gs, off_max, off_lse, off_rows, off_flags, total;
};
bool in_envelope(int64_t nq, int64_t nc, int d) {
    return nq >= 1 && nq <= 1024 && nc >= nq && nc <= 2048 && d >= 128 && d <= 1024 && d % 4 == 0;
}
Layout layout(int64_t nq, int64_t nc) {
    Layout L;
    const size_t mat = align_up(sizeof(float) * (size_t)nq * (size_t)nc, 256), vec = align_up(sizeof(float) * (size_t)nq, 256);
    L.off_gs = mat;
    L.off_max = 2 * mat;
    L.off_lse = L.off_max + vec;
    L.off_rows = L.off_lse + vec;
    L.off_flags = L.off_rows + vec;
    L.total = L.off_flags + vec;
    return L;
}
const char *check_common(const void *q, const void *ctx, const void *pos, int64_t nq, int64_t nc, int d, const void *ws, size_t ws_bytes) {
    if (!q || !ctx || !pos) return "null pointer";
    if (!in_envelope(nq, nc, d)) return "shape outside 1 <= nq <= 1024, nq <= nc <= 2048, 128 <= d <= 1024, d % 4 == 0";
    if (!ws || (uintptr_t)ws % 16) return "null or unaligned workspace";
    if (ws_bytes < layout(nq, nc).total) return "workspace too small";
    return nullptr;
}

}  // namespace
}  // namespace ance

extern "C" size_t ance_inbatch_nll_workspace_bytes(int64_t nq, int64_t nc, int d) {
    using namespace ance;
    return in_envelope(nq, nc, d) ? layout(nq, nc).total : 0;
}

extern "C" int ance_inbatch_nll_forward(const float *d_q, const float *d_ctx, const int64_t *d_positive_idx, int64_t nq, int64_t nc, int d,
                                        float *d_loss_mean, int64_t *d_counts, void *d_workspace, size_t workspace_bytes, void *stream) {
    using namespace ance;
    const char *fn = "ance_inbatch_nll_forward";
    if (!d_loss_mean || !d_counts) return refuse(fn, "null pointer");
    if (const char *why = check_common(d_q, d_ctx, d_positive_idx, nq, nc, d, d_workspace, workspace_bytes)) return refuse(fn, why);
    const Layout L = layout(nq, nc);
    char *ws = (char *)d_workspace;
    float *S = (float *)ws, *row_max = (float *)(ws + L.off_max), *log_sum = (float *)(ws + L.off_lse), *rows = (float *)(ws + L.off_rows);
    int32_t *flags = (int32_t *)(ws + L.off_flags);
    hipStream_t st = (hipStream_t)stream;
    launch_gemm<true, true>(d_q, d_ctx, S, (int)nq, (int)nc, d, st);
    hipLaunchKernelGGL(inbatch_rows_kernel, dim3((unsigned)nq), dim3(256), 0, st, (const float *)S, d_positive_idx, (int)nc, row_max, log_sum,
                       rows, flags);
    hipLaunchKernelGGL(inbatch_reduce_kernel, dim3(1), dim3(1024), 0, st, (const float *)rows, (const int32_t *)flags, (int)nq, d_loss_mean,
                       d_counts);
    return check_launch(fn);
}

extern "C" int ance_inbatch_nll_backward(const float *d_q, const float *d_ctx, const int64_t *d_positive_idx, int64_t nq, int64_t nc, int d,
                                         const float *d_grad_output, float *d_gq, float *d_gctx, void *d_workspace, size_t workspace_bytes,
                                         void *stream) {
    using namespace ance;
    const char *fn = "ance_inbatch_nll_backward";
    if (!d_grad_output || !d_gq || !d_gctx) return refuse(fn, "null pointer");
    if (const char *why = check_common(d_q, d_ctx, d_positive_idx, nq, nc, d, d_workspace, workspace_bytes)) return refuse(fn, why);
    const Layout L = layout(nq, nc);
    char *ws = (char *)d_workspace;
    const float *S = (const float *)ws, *row_max = (const float *)(ws + L.off_max), *log_sum = (const float *)(ws + L.off_lse);
    float *gS = (float *)(ws + L.off_gs);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(inbatch_gs_kernel, dim3((unsigned)nq), dim3(256), 0, st, S, row_max, log_sum, d_positive_idx, (int)nq, (int)nc,
                       d_grad_output, gS);
    launch_gemm<true, false>((const float *)gS, d_ctx, d_gq, (int)nq, d, (int)nc, st);    // gq [nq, d] = gS [nq][nc] . ctx [nc][d]
    launch_gemm<false, false>((const float *)gS, d_q, d_gctx, (int)nc, d, (int)nq, st);   // gctx [nc, d] = gS^T ([nq][nc]) . q [nq][d]
    return check_launch(fn);
}
