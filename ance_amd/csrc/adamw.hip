// Fused multi-tensor AdamW step (include/ance_amd.h: ance_adamw_step): transformers 2.3.0 optimization.py AdamW.step -- the optimizer
// drivers/run_ann_dpr.py builds by default and run_ann.py / run_warmup.py build for --optimizer adamW; a Python loop of about ten
// small launches per parameter tensor there -- for every tensor of the call, with no host synchronisation.  Unlike LAMB there is no
// trust ratio, so no norm stands between the moments and the update and the step is ONE elementwise pass; unlike LAMB there is a
// bias correction, so the step count enters the arithmetic and lives on the device, per tensor, where a skipped step leaves it.
//   prep     (one workgroup of 1024; one thread per tensor)  t = *step + 1; ss = float32(lr sqrt(1 - beta2^t) / (1 - beta1^t)) and
//            the decay factor float32(-lr wd) in fp64, as the reference's Python doubles -> the workspace; *step <- t.  A skipped
//            step (found_inf) writes nothing of it and one thread adds 1 to *d_skipped with an ordinary load, add and store.
//            With clipping the same workgroup first adds the chunk sums of gnorm in chunk order: *d_grad_norm and coef exactly as
//            ance_lamb_step_clipped forms them (multi_tensor.h: grad_total), also in a skipped step.
//   update   (one workgroup per 16,384-element chunk, 256 threads, float4 accesses, 4 per array in flight)
//            m <- b1 m + (1 - b1) g; v <- b2 v + (1 - b2) g g; p <- p - ss (m / (sqrt(v) + eps)); p <- p + float32(-lr wd) p on the
//            UPDATED p when wd > 0: reads p, g, m, v (16 B / element), writes p, m, v (12 B).  Returns before any store in a
//            skipped step.
//   gnorm    (clipping only, in front; one workgroup per chunk; multi_tensor.hip)  reads g only (4 B); the chunk's sum of g^2 (fp64)
//            to its slot
// Launches: TWO without clipping (prep, update: 28 B per element), THREE with it (gnorm, prep, update: 32 B per element), under
// loss scaling too (unscale in registers, skip on the device: the arithmetic of ance_lamb_step_amp).  No atomics and a fixed
// summation order: the same inputs give the same bits.  Division and sqrtf are the IEEE ones, as in lamb.hip.
// ance_adamw_step_scaled (a loss scaler that hands no flag in): always the three launches; prep (adamw_prep_scaled_kernel) totals
// first, stores the overflow flag from the fp64 total and only then decides whether the step counts advance.
//
// Here: AdamW's arithmetic, prep and update, its group rows and its entry point.  The walk of a workgroup over its chunk and the
// device tensor row are multi_tensor.h's; the checks and the fill of the tables, the staging pool and gnorm are multi_tensor.hip's,
// shared with lamb.hip.
#include "multi_tensor.h"

namespace ance {
namespace {

using mt::align16;
using mt::DevTensor;
constexpr int THREADS = mt::THREADS;

struct AdamwDevGroup {
    double lr, beta1, beta2, wd;        // the reference's Python doubles: the step size and the decay factor are formed from these
    float b1, omb1, b2, omb2, eps;      // rounded to fp32 as torch does for a scalar: the moment updates and the denominator
    int32_t has_wd;
    const double *d_lr;                 // the learning rate as a device fp64 scalar (a resident plan's group with a tensor lr), or null: lr
};
struct AdamwScalars {  // per tensor, written by prep
    float neg_ss, decay;
};

// one element: the moments, then the parameter
__device__ __forceinline__ float adamw_elem(float p, float g, float &m, float &v, const AdamwDevGroup &G, AdamwScalars S) {
    m = __builtin_fmaf(G.omb1, g, m * G.b1);
    v = __builtin_fmaf(G.omb2 * g, g, v * G.b2);
    p = __builtin_fmaf(S.neg_ss, m / (sqrtf(v) + G.eps), p);
    if (G.has_wd) p = __builtin_fmaf(S.decay, p, p);
    return p;
}

// prep, one thread per tensor of an applied step: t, ss and the decay factor -> scalars[t]; *step <- t
__device__ __forceinline__ void adamw_prep_tensors(const AdamwDevGroup *groups, const DevTensor *tensors, int n_tensors, int correct_bias,
                                                   AdamwScalars *scalars) {
    for (int t = threadIdx.x; t < n_tensors; t += 1024) {
        const DevTensor T = tensors[t];
        if (T.numel == 0) continue;  // its step is neither read nor written
        const AdamwDevGroup G = groups[T.group];
        const float t1 = T.step[0] + 1.0f;  // exact up to 2^24 steps
        const double lr = G.d_lr ? G.d_lr[0] : G.lr;  // the same fp64 value either way, so the same ss and decay
        double ss = lr;
        if (correct_bias) ss = ss * sqrt(1.0 - pow(G.beta2, (double)t1)) / (1.0 - pow(G.beta1, (double)t1));
        AdamwScalars S;
        S.neg_ss = (float)(-ss);
        S.decay = (float)(-lr * G.wd);
        scalars[t] = S;
        T.step[0] = t1;
    }
}

// CLIP: the gradient total and the clip factor first (one workgroup: multi_tensor.h).  Then one thread per tensor.
template <bool CLIP>
__global__ void __launch_bounds__(1024) adamw_prep_kernel(const AdamwDevGroup *groups, const DevTensor *tensors, int n_tensors,
                                                          int correct_bias, AdamwScalars *scalars, const double *gpartial,
                                                          int n_chunks, float max_norm, float *grad_norm, float *coef,
                                                          const float *found_inf, int64_t *skipped) {
    __shared__ double s[CLIP ? 1024 : 1];
    if (CLIP) mt::grad_total(gpartial, n_chunks, max_norm, grad_norm, coef, s);
    if (mt::skip(found_inf)) {
        if (threadIdx.x == 0 && skipped) skipped[0] = skipped[0] + 1;
        return;
    }
    adamw_prep_tensors(groups, tensors, n_tensors, correct_bias, scalars);
}

// prep of ance_adamw_step_scaled: the gradient total always comes first and the step's own overflow flag with it (multi_tensor.h:
// grad_total_flag; thread 0 stores *found_inf), and only then is it decided whether the step counts advance.
template <bool CLIP>
__global__ void __launch_bounds__(1024) adamw_prep_scaled_kernel(const AdamwDevGroup *groups, const DevTensor *tensors, int n_tensors,
                                                                 int correct_bias, AdamwScalars *scalars, const double *gpartial,
                                                                 int n_chunks, float max_norm, float *grad_norm, float *coef,
                                                                 float *found_inf, int64_t *skipped) {
    __shared__ double s[1024];
    if (mt::grad_total_flag<CLIP>(gpartial, n_chunks, max_norm, grad_norm, coef, found_inf, s)) {
        if (threadIdx.x == 0 && skipped) skipped[0] = skipped[0] + 1;
        return;
    }
    adamw_prep_tensors(groups, tensors, n_tensors, correct_bias, scalars);
}

// CLIP: every gradient element is multiplied by *coef before it enters m and v; UNSCALE: by the inverse of *grad_scale before that.
// found_inf (nullable): a skipped step returns before any store.
template <bool CLIP, bool UNSCALE>
__global__ void __launch_bounds__(THREADS) adamw_update_kernel(const AdamwDevGroup *groups, const DevTensor *tensors,
                                                               const int32_t *chunk_tensor, const AdamwScalars *scalars,
                                                               const float *coef, const float *grad_scale, const float *found_inf) {
    if (mt::skip(found_inf)) return;
    const float cf = CLIP ? coef[0] : 1.0f;
    const float inv = UNSCALE ? mt::inv_scale(grad_scale) : 1.0f;
    const int t = chunk_tensor[blockIdx.x];
    const DevTensor T = tensors[t];
    const AdamwDevGroup G = groups[T.group];
    const AdamwScalars S = scalars[t];
    float *a[4];
    const int len = mt::chunk_of(T, a);
    mt::stream_chunk<0b1111, 0b1101>(a, len, T.vec, [&](float(&x)[4]) {
        x[0] = adamw_elem(x[0], mt::grad<CLIP, UNSCALE>(x[1], inv, cf), x[2], x[3], G, S);
    });
}

// workspace: [groups][tensors][chunk -> tensor] (staged from the host in one copy: multi_tensor.h) [scalars per tensor]; clipping
// appends [fp64 g^2 per chunk][coef (fp32, 16 bytes)]
size_t workspace_bytes_for(int n_tensors, int n_groups, int64_t n_chunks, bool clip) {
    size_t b = mt::staged(sizeof(AdamwDevGroup), n_tensors, n_groups, n_chunks).end + align16(sizeof(AdamwScalars) * (size_t)n_tensors);
    if (clip) b += align16(sizeof(double) * (size_t)n_chunks) + 16;
    return b;
}

void adamw_group_row(void *row, const AnceLambGroup &a, const double *d_lr) {
    AdamwDevGroup &G = *(AdamwDevGroup *)row;
    G.d_lr = d_lr;
    G.lr = a.lr;
    G.beta1 = a.beta1;
    G.beta2 = a.beta2;
    G.wd = a.weight_decay;
    G.b1 = (float)a.beta1;
    G.omb1 = (float)(1.0 - a.beta1);
    G.b2 = (float)a.beta2;
    G.omb2 = (float)(1.0 - a.beta2);
    G.eps = (float)a.eps;
    G.has_wd = a.weight_decay > 0.0;
}

template <bool CLIP>
void launch_update(bool unscale, int64_t n_chunks, hipStream_t st, const AdamwDevGroup *dG, const DevTensor *dT, const int32_t *dC,
                   const AdamwScalars *dS, const float *dCoef, const float *grad_scale, const float *found_inf) {
    if (unscale)
        hipLaunchKernelGGL((adamw_update_kernel<CLIP, true>), dim3((unsigned)n_chunks), dim3(THREADS), 0, st, dG, dT, dC, dS, dCoef,
                           grad_scale, found_inf);
    else
        hipLaunchKernelGGL((adamw_update_kernel<CLIP, false>), dim3((unsigned)n_chunks), dim3(THREADS), 0, st, dG, dT, dC, dS, dCoef,
                           (const float *)nullptr, found_inf);
}

// the launches of a step whose tables stand at the head of ws (layout L): two, or three with the clip.  flag_out (ance_adamw_step_scaled;
// then d_found_inf == flag_out and ws has the clipped layout): three, the step writes the flag itself
int adamw_launch(const char *fn, int n_tensors, int64_t n_chunks, const mt::Staged &L, int correct_bias, bool clip, double max_grad_norm,
                 const float *d_grad_scale, const float *d_found_inf, float *d_grad_norm, int64_t *d_skipped, char *ws, hipStream_t st,
                 float *flag_out = nullptr) {
    const AdamwDevGroup *dG = (const AdamwDevGroup *)ws;
    const DevTensor *dT = (const DevTensor *)(ws + L.tensors);
    const int32_t *dC = (const int32_t *)(ws + L.chunk_tensor);
    AdamwScalars *dS = (AdamwScalars *)(ws + L.end);
    if (flag_out) {
        double *dGP = (double *)(ws + L.end + align16(sizeof(AdamwScalars) * (size_t)n_tensors));
        float *dCoef = (float *)((char *)dGP + align16(sizeof(double) * (size_t)n_chunks));
        mt::launch_gnorm(n_chunks, st, dT, dC, dGP, d_grad_scale);
        if (clip) {
            hipLaunchKernelGGL(adamw_prep_scaled_kernel<true>, dim3(1), dim3(1024), 0, st, dG, dT, n_tensors, correct_bias ? 1 : 0, dS,
                               (const double *)dGP, (int)n_chunks, (float)max_grad_norm, d_grad_norm, dCoef, flag_out, d_skipped);
            if (n_chunks > 0) launch_update<true>(true, n_chunks, st, dG, dT, dC, dS, dCoef, d_grad_scale, d_found_inf);
        } else {
            hipLaunchKernelGGL(adamw_prep_scaled_kernel<false>, dim3(1), dim3(1024), 0, st, dG, dT, n_tensors, correct_bias ? 1 : 0, dS,
                               (const double *)dGP, (int)n_chunks, 0.0f, (float *)nullptr, (float *)nullptr, flag_out, d_skipped);
            if (n_chunks > 0) launch_update<false>(true, n_chunks, st, dG, dT, dC, dS, nullptr, d_grad_scale, d_found_inf);
        }
    } else if (clip) {
        double *dGP = (double *)(ws + L.end + align16(sizeof(AdamwScalars) * (size_t)n_tensors));
        float *dCoef = (float *)((char *)dGP + align16(sizeof(double) * (size_t)n_chunks));
        mt::launch_gnorm(n_chunks, st, dT, dC, dGP, d_grad_scale);
        hipLaunchKernelGGL(adamw_prep_kernel<true>, dim3(1), dim3(1024), 0, st, dG, dT, n_tensors, correct_bias ? 1 : 0, dS,
                           (const double *)dGP, (int)n_chunks, (float)max_grad_norm, d_grad_norm, dCoef, d_found_inf, d_skipped);
        if (n_chunks > 0) launch_update<true>(d_grad_scale != nullptr, n_chunks, st, dG, dT, dC, dS, dCoef, d_grad_scale, d_found_inf);
    } else {
        hipLaunchKernelGGL(adamw_prep_kernel<false>, dim3(1), dim3(1024), 0, st, dG, dT, n_tensors, correct_bias ? 1 : 0, dS,
                           (const double *)nullptr, 0, 0.0f, (float *)nullptr, (float *)nullptr, d_found_inf, d_skipped);
        if (n_chunks > 0) launch_update<false>(d_grad_scale != nullptr, n_chunks, st, dG, dT, dC, dS, nullptr, d_grad_scale, d_found_inf);
    }
    return check_launch(fn);
}

}  // namespace
}  // namespace ance

extern "C" size_t ance_adamw_workspace_bytes(int n_tensors, int n_groups, int64_t total_numel, int clip) {
    using namespace ance;
    if (n_tensors < 0 || n_groups < 1 || total_numel < 0) return 0;
    const int64_t chunks = mt::max_chunks(n_tensors, total_numel);
    if (chunks > (int64_t)INT32_MAX) return 0;
    return workspace_bytes_for(n_tensors, n_groups, chunks, clip != 0);
}

extern "C" int ance_adamw_step(const AnceAdamwTensor *h_tensors, int n_tensors, const AnceLambGroup *h_groups, int n_groups,
                               int correct_bias, double max_grad_norm, const float *d_grad_scale, const float *d_found_inf,
                               float *d_grad_norm, int64_t *d_skipped, void *d_workspace, size_t workspace_bytes, void *stream) {
    using namespace ance;
    const char *fn = "ance_adamw_step";
    if (!(max_grad_norm >= 0.0) || !(max_grad_norm < (double)INFINITY))
        return refuse(fn, "max_grad_norm not 0 or a positive finite number");
    const bool clip = max_grad_norm != 0.0;
    if (clip && n_tensors > 0 && !d_grad_norm) return refuse(fn, "null d_grad_norm");
    if (n_tensors < 0) return refuse(fn, "n_tensors < 0");
    if (n_tensors == 0) return ANCE_OK;
    if (!h_tensors || !h_groups) return refuse(fn, "null table");
    if (n_groups < 1) return refuse(fn, "n_groups < 1");
    int64_t n_chunks = 0;
    if (const int e = mt::count_chunks(fn, h_tensors, n_tensors, n_groups, &n_chunks)) return e;
    const size_t need = workspace_bytes_for(n_tensors, n_groups, n_chunks, clip);
    if (!d_workspace || (uintptr_t)d_workspace % 16) return refuse(fn, "null or unaligned workspace");
    if (workspace_bytes < need) return refuse(fn, "workspace too small");

    const mt::Staged L = mt::staged(sizeof(AdamwDevGroup), n_tensors, n_groups, n_chunks);
    hipStream_t st = (hipStream_t)stream;
    char *ws = (char *)d_workspace;
    if (const int e = mt::stage_tables(fn, h_tensors, n_tensors, h_groups, n_groups, sizeof(AdamwDevGroup), adamw_group_row, L, ws, st))
        return e;
    return adamw_launch(fn, n_tensors, n_chunks, L, correct_bias, clip, max_grad_norm, d_grad_scale, d_found_inf, d_grad_norm, d_skipped,
                        ws, st);
}

// ---- the resident plan (include/ance_amd.h; as lamb.hip's)
extern "C" size_t ance_adamw_plan_table_bytes(int n_tensors, int n_groups, int64_t total_numel) {
    using namespace ance;
    if (n_tensors < 0 || n_groups < 1 || total_numel < 0) return 0;
    const int64_t chunks = mt::max_chunks(n_tensors, total_numel);
    if (chunks > (int64_t)INT32_MAX) return 0;
    return mt::staged(sizeof(AdamwDevGroup), n_tensors, n_groups, chunks).end;
}

extern "C" int ance_adamw_plan_build(const AnceAdamwTensor *h_tensors, int n_tensors, const AnceLambGroup *h_groups,
                                     const double *const *d_lrs, int n_groups, void *h_tables, size_t h_tables_bytes,
                                     int64_t *n_chunks_out, size_t *table_bytes_out) {
    using namespace ance;
    const char *fn = "ance_adamw_plan_build";
    if (n_tensors < 1) return refuse(fn, "n_tensors < 1");
    if (!h_tensors || !h_groups) return refuse(fn, "null table");
    if (n_groups < 1) return refuse(fn, "n_groups < 1");
    int64_t n_chunks = 0;
    if (const int e = mt::count_chunks(fn, h_tensors, n_tensors, n_groups, &n_chunks)) return e;
    if (!h_tables || !n_chunks_out || !table_bytes_out) return refuse(fn, "null pointer");
    const mt::Staged L = mt::staged(sizeof(AdamwDevGroup), n_tensors, n_groups, n_chunks);
    if (h_tables_bytes < L.end) return refuse(fn, "h_tables too small");
    mt::fill_tables(h_tensors, n_tensors, h_groups, d_lrs, n_groups, sizeof(AdamwDevGroup), adamw_group_row, L, (char *)h_tables);
    *n_chunks_out = n_chunks;
    *table_bytes_out = L.end;
    return ANCE_OK;
}

extern "C" int ance_adamw_step_planned(int n_tensors, int n_groups, int64_t n_chunks, int correct_bias, double max_grad_norm,
                                       const float *d_grad_scale, const float *d_found_inf, float *d_grad_norm, int64_t *d_skipped,
                                       void *d_workspace, size_t workspace_bytes, void *stream) {
    using namespace ance;
    const char *fn = "ance_adamw_step_planned";
    if (n_tensors < 1 || n_groups < 1 || n_chunks < 0 || n_chunks > (int64_t)INT32_MAX) return refuse(fn, "table sizes out of range");
    if (!(max_grad_norm >= 0.0) || !(max_grad_norm < (double)INFINITY))
        return refuse(fn, "max_grad_norm not 0 or a positive finite number");
    const bool clip = max_grad_norm != 0.0;
    if (clip && !d_grad_norm) return refuse(fn, "null d_grad_norm");
    if (!d_workspace || (uintptr_t)d_workspace % 16) return refuse(fn, "null or unaligned workspace");
    if (workspace_bytes < workspace_bytes_for(n_tensors, n_groups, n_chunks, clip)) return refuse(fn, "workspace too small");
    const mt::Staged L = mt::staged(sizeof(AdamwDevGroup), n_tensors, n_groups, n_chunks);
    return adamw_launch(fn, n_tensors, n_chunks, L, correct_bias, clip, max_grad_norm, d_grad_scale, d_found_inf, d_grad_norm, d_skipped,
                        (char *)d_workspace, (hipStream_t)stream);
}

// ance_adamw_step_planned for a caller that has no overflow flag to hand in: the step derives it (include/ance_amd.h)
extern "C" int ance_adamw_step_scaled(int n_tensors, int n_groups, int64_t n_chunks, int correct_bias, double max_grad_norm,
                                      const float *d_grad_scale, float *d_found_inf, float *d_grad_norm, int64_t *d_skipped,
                                      void *d_workspace, size_t workspace_bytes, void *stream) {
    using namespace ance;
    const char *fn = "ance_adamw_step_scaled";
    if (n_tensors < 1 || n_groups < 1 || n_chunks < 0 || n_chunks > (int64_t)INT32_MAX) return refuse(fn, "table sizes out of range");
    if (!(max_grad_norm >= 0.0) || !(max_grad_norm < (double)INFINITY))
        return refuse(fn, "max_grad_norm not 0 or a positive finite number");
    const bool clip = max_grad_norm != 0.0;
    if (clip && !d_grad_norm) return refuse(fn, "null d_grad_norm");
    if (!d_grad_scale) return refuse(fn, "null d_grad_scale");
    if (!d_found_inf) return refuse(fn, "null d_found_inf");
    if (!d_workspace || (uintptr_t)d_workspace % 16) return refuse(fn, "null or unaligned workspace");
    if (workspace_bytes < workspace_bytes_for(n_tensors, n_groups, n_chunks, true)) return refuse(fn, "workspace too small");
    const mt::Staged L = mt::staged(sizeof(AdamwDevGroup), n_tensors, n_groups, n_chunks);
    return adamw_launch(fn, n_tensors, n_chunks, L, correct_bias, clip, max_grad_norm, d_grad_scale, d_found_inf, d_grad_norm, d_skipped,
                        (char *)d_workspace, (hipStream_t)stream, d_found_inf);
}
