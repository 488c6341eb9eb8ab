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
//   gnorm    (clipping only, in front; one workgroup per chunk)  reads g only (4 B); the chunk's sum of g^2 (fp64) to its slot
// Launches: TWO without clipping (prep, update: 28 B per element), THREE with it (gnorm, prep, update: 32 B per element), under
// loss scaling too (unscale in registers, skip on the device: the arithmetic of ance_lamb_step_amp).  No atomics and a fixed
// summation order: the same inputs give the same bits.  Division and sqrtf are the IEEE ones, as in lamb.hip.
#include "multi_tensor.h"

namespace ance {
namespace {

using mt::align16;
using mt::gf32x4;
using mt::gfloat;
constexpr int CHUNK = mt::CHUNK, THREADS = mt::THREADS, UNROLL = mt::UNROLL;

struct AdamwDevGroup {
    double lr, beta1, beta2, wd;        // the reference's Python doubles: the step size and the decay factor are formed from these
    float b1, omb1, b2, omb2, eps;      // rounded to fp32 as torch does for a scalar: the moment updates and the denominator
    int32_t has_wd;
};
struct AdamwDevTensor {
    float *p;
    const float *g;
    float *m, *v;
    float *step;
    int64_t numel;
    int32_t chunk0, n_chunks, group, vec;
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

// CLIP: the gradient total and the clip factor first (one workgroup: multi_tensor.h).  Then one thread per tensor.
template <bool CLIP>
__global__ void __launch_bounds__(1024) adamw_prep_kernel(const AdamwDevGroup *groups, const AdamwDevTensor *tensors, int n_tensors,
                                                          int correct_bias, AdamwScalars *scalars, const double *gpartial,
                                                          int n_chunks, float max_norm, float *grad_norm, float *coef,
                                                          const float *found_inf, int64_t *skipped) {
    __shared__ double s[CLIP ? 1024 : 1];
    if (CLIP) mt::grad_total(gpartial, n_chunks, max_norm, grad_norm, coef, s);
    if (mt::skip(found_inf)) {
        if (threadIdx.x == 0 && skipped) skipped[0] = skipped[0] + 1;
        return;
    }
    for (int t = threadIdx.x; t < n_tensors; t += 1024) {
        const AdamwDevTensor T = tensors[t];
        if (T.numel == 0) continue;  // its step is neither read nor written
        const AdamwDevGroup G = groups[T.group];
        const float t1 = T.step[0] + 1.0f;  // exact up to 2^24 steps
        double ss = G.lr;
        if (correct_bias) ss = ss * sqrt(1.0 - pow(G.beta2, (double)t1)) / (1.0 - pow(G.beta1, (double)t1));
        AdamwScalars S;
        S.neg_ss = (float)(-ss);
        S.decay = (float)(-G.lr * G.wd);
        scalars[t] = S;
        T.step[0] = t1;
    }
}

// CLIP: every gradient element is multiplied by *coef before it enters m and v; UNSCALE: by the inverse of *grad_scale before that.
// found_inf (nullable): a skipped step returns before any store.
template <bool CLIP, bool UNSCALE>
__global__ void __launch_bounds__(THREADS) adamw_update_kernel(const AdamwDevGroup *groups, const AdamwDevTensor *tensors,
                                                               const int32_t *chunk_tensor, const AdamwScalars *scalars,
                                                               const float *coef, const float *grad_scale, const float *found_inf) {
    if (mt::skip(found_inf)) return;
    const int tid = threadIdx.x;
    const float cf = CLIP ? coef[0] : 1.0f;
    const float inv = UNSCALE ? mt::inv_scale(grad_scale) : 1.0f;
    const int t = chunk_tensor[blockIdx.x];
    const AdamwDevTensor T = tensors[t];
    const AdamwDevGroup G = groups[T.group];
    const AdamwScalars S = scalars[t];
    const int64_t base = (int64_t)(blockIdx.x - T.chunk0) * CHUNK;
    const int len = (int)min((int64_t)CHUNK, T.numel - base);
    gfloat *p = (gfloat *)(T.p + base), *m = (gfloat *)(T.m + base), *v = (gfloat *)(T.v + base);
    const gfloat *g = (const gfloat *)(T.g + base);
    int done = 0;
    if (T.vec) {  // every pointer 16-byte aligned (chunk starts are multiples of 4 elements)
        const int n4 = len >> 2;
        const gf32x4 *g4 = (const gf32x4 *)g;
        gf32x4 *p4 = (gf32x4 *)p, *m4 = (gf32x4 *)m, *v4 = (gf32x4 *)v;
        for (int i0 = tid; i0 < n4; i0 += THREADS * UNROLL) {
            f32x4 P[UNROLL], Gr[UNROLL], M[UNROLL], V[UNROLL];
#pragma unroll
            for (int k = 0; k < UNROLL; ++k) {
                const int i = i0 + k * THREADS;
                if (i < n4) { P[k] = p4[i]; Gr[k] = g4[i]; M[k] = m4[i]; V[k] = v4[i]; }
            }
#pragma unroll
            for (int k = 0; k < UNROLL; ++k) {
                const int i = i0 + k * THREADS;
                if (i < n4) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        float mj = M[k][j], vj = V[k][j];
                        P[k][j] = adamw_elem(P[k][j], mt::grad<CLIP, UNSCALE>(Gr[k][j], inv, cf), mj, vj, G, S);
                        M[k][j] = mj;
                        V[k][j] = vj;
                    }
                    p4[i] = P[k];
                    m4[i] = M[k];
                    v4[i] = V[k];
                }
            }
        }
        done = n4 * 4;
    }
    for (int e = done + tid; e < len; e += THREADS) {  // scalar tail (or the whole chunk of an unaligned tensor)
        float mj = m[e], vj = v[e];
        p[e] = adamw_elem(p[e], mt::grad<CLIP, UNSCALE>(g[e], inv, cf), mj, vj, G, S);
        m[e] = mj;
        v[e] = vj;
    }
}

// workspace: [groups][tensors][chunk -> tensor] (staged from the host in one copy) [scalars per tensor]; clipping appends
// [fp64 g^2 per chunk][coef (fp32, 16 bytes)]
size_t staged_bytes(int n_tensors, int n_groups, int64_t n_chunks) {
    return align16(sizeof(AdamwDevGroup) * (size_t)n_groups) + align16(sizeof(AdamwDevTensor) * (size_t)n_tensors) +
           align16(sizeof(int32_t) * (size_t)n_chunks);
}
size_t workspace_bytes_for(int n_tensors, int n_groups, int64_t n_chunks, bool clip) {
    size_t b = staged_bytes(n_tensors, n_groups, n_chunks) + align16(sizeof(AdamwScalars) * (size_t)n_tensors);
    if (clip) b += align16(sizeof(double) * (size_t)n_chunks) + 16;
    return b;
}

int adamw_refuse(const char *why) {
    char buf[160];
    snprintf(buf, sizeof(buf), "ance_adamw_step: invalid argument (%s)", why);
    set_last_error(buf);
    return ANCE_E_INVALID;
}

template <bool CLIP>
void launch_update(bool unscale, int64_t n_chunks, hipStream_t st, const AdamwDevGroup *dG, const AdamwDevTensor *dT, const int32_t *dC,
                   const AdamwScalars *dS, const float *dCoef, const float *grad_scale, const float *found_inf) {
    if (unscale)
        hipLaunchKernelGGL((adamw_update_kernel<CLIP, true>), dim3((unsigned)n_chunks), dim3(THREADS), 0, st, dG, dT, dC, dS, dCoef,
                           grad_scale, found_inf);
    else
        hipLaunchKernelGGL((adamw_update_kernel<CLIP, false>), dim3((unsigned)n_chunks), dim3(THREADS), 0, st, dG, dT, dC, dS, dCoef,
                           (const float *)nullptr, found_inf);
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
    if (!(max_grad_norm >= 0.0) || !(max_grad_norm < (double)INFINITY))
        return adamw_refuse("max_grad_norm not 0 or a positive finite number");
    const bool clip = max_grad_norm != 0.0;
    if (clip && n_tensors > 0 && !d_grad_norm) return adamw_refuse("null d_grad_norm");
    if (n_tensors < 0) return adamw_refuse("n_tensors < 0");
    if (n_tensors == 0) return ANCE_OK;
    if (!h_tensors || !h_groups) return adamw_refuse("null table");
    if (n_groups < 1) return adamw_refuse("n_groups < 1");
    int64_t n_chunks = 0;
    for (int t = 0; t < n_tensors; ++t) {
        const AnceAdamwTensor &T = h_tensors[t];
        if (T.group < 0 || T.group >= n_groups) return adamw_refuse("group index out of range");
        if (T.numel < 0) return adamw_refuse("numel < 0");
        if (T.numel > 0 && (!T.p || !T.g || !T.m || !T.v)) return adamw_refuse("null tensor pointer");
        if (T.numel > 0 && !T.step) return adamw_refuse("null step of a tensor with elements");
        n_chunks += (T.numel + CHUNK - 1) / CHUNK;
        if (n_chunks > (int64_t)INT32_MAX) return adamw_refuse("too many elements");
    }
    const size_t need = workspace_bytes_for(n_tensors, n_groups, n_chunks, clip);
    if (!d_workspace || (uintptr_t)d_workspace % 16) return adamw_refuse("null or unaligned workspace");
    if (workspace_bytes < need) return adamw_refuse("workspace too small");

    const size_t off_t = align16(sizeof(AdamwDevGroup) * (size_t)n_groups);
    const size_t off_c = off_t + align16(sizeof(AdamwDevTensor) * (size_t)n_tensors);
    const size_t off_s = staged_bytes(n_tensors, n_groups, n_chunks);
    const size_t off_g = off_s + align16(sizeof(AdamwScalars) * (size_t)n_tensors);
    hipStream_t st = (hipStream_t)stream;
    char *ws = (char *)d_workspace;
    {
        std::lock_guard<std::mutex> lock(mt::g_stage_mu);
        const int si = mt::stage_acquire(off_s);
        if (si < 0) {
            set_last_error("ance_adamw_step: pinned staging buffer");
            return ANCE_E_NOMEM;
        }
        mt::Staging &S = mt::g_stage[si];
        char *h = (char *)S.h;
        AdamwDevGroup *G = (AdamwDevGroup *)h;
        for (int i = 0; i < n_groups; ++i) {
            const AnceLambGroup &a = h_groups[i];
            G[i].lr = a.lr;
            G[i].beta1 = a.beta1;
            G[i].beta2 = a.beta2;
            G[i].wd = a.weight_decay;
            G[i].b1 = (float)a.beta1;
            G[i].omb1 = (float)(1.0 - a.beta1);
            G[i].b2 = (float)a.beta2;
            G[i].omb2 = (float)(1.0 - a.beta2);
            G[i].eps = (float)a.eps;
            G[i].has_wd = a.weight_decay > 0.0;
        }
        AdamwDevTensor *T = (AdamwDevTensor *)(h + off_t);
        int32_t *ct = (int32_t *)(h + off_c);
        int32_t c = 0;
        for (int t = 0; t < n_tensors; ++t) {
            const AnceAdamwTensor &a = h_tensors[t];
            T[t].p = a.p;
            T[t].g = a.g;
            T[t].m = a.m;
            T[t].v = a.v;
            T[t].step = a.step;
            T[t].numel = a.numel;
            T[t].group = a.group;
            T[t].chunk0 = c;
            T[t].n_chunks = (int32_t)((a.numel + CHUNK - 1) / CHUNK);
            T[t].vec = ((uintptr_t)a.p | (uintptr_t)a.g | (uintptr_t)a.m | (uintptr_t)a.v) % 16 == 0;
            for (int32_t k = 0; k < T[t].n_chunks; ++k) ct[c++] = t;
        }
        const int sent = mt::stage_send(S, ws, off_s, st);
        if (sent) return check_launch(sent == 1 ? "ance_adamw_step: tables" : "ance_adamw_step: staging event");
    }
    const AdamwDevGroup *dG = (const AdamwDevGroup *)ws;
    const AdamwDevTensor *dT = (const AdamwDevTensor *)(ws + off_t);
    const int32_t *dC = (const int32_t *)(ws + off_c);
    AdamwScalars *dS = (AdamwScalars *)(ws + off_s);
    if (clip) {
        double *dGP = (double *)(ws + off_g);
        float *dCoef = (float *)((char *)dGP + align16(sizeof(double) * (size_t)n_chunks));
        if (n_chunks > 0) {
            if (d_grad_scale)
                hipLaunchKernelGGL((mt::gnorm_kernel<AdamwDevTensor, true>), dim3((unsigned)n_chunks), dim3(THREADS), 0, st, dT, dC, dGP,
                                   d_grad_scale);
            else
                hipLaunchKernelGGL((mt::gnorm_kernel<AdamwDevTensor, false>), dim3((unsigned)n_chunks), dim3(THREADS), 0, st, dT, dC, dGP,
                                   (const float *)nullptr);
        }
        hipLaunchKernelGGL(adamw_prep_kernel<true>, dim3(1), dim3(1024), 0, st, dG, dT, n_tensors, correct_bias ? 1 : 0, dS,
                           (const double *)dGP, (int)n_chunks, (float)max_grad_norm, d_grad_norm, dCoef, d_found_inf, d_skipped);
        if (n_chunks > 0) launch_update<true>(d_grad_scale != nullptr, n_chunks, st, dG, dT, dC, dS, dCoef, d_grad_scale, d_found_inf);
    } else {
        hipLaunchKernelGGL(adamw_prep_kernel<false>, dim3(1), dim3(1024), 0, st, dG, dT, n_tensors, correct_bias ? 1 : 0, dS,
                           (const double *)nullptr, 0, 0.0f, (float *)nullptr, (float *)nullptr, d_found_inf, d_skipped);
        if (n_chunks > 0) launch_update<false>(d_grad_scale != nullptr, n_chunks, st, dG, dT, dC, dS, nullptr, d_grad_scale, d_found_inf);
    }
    return check_launch("ance_adamw_step");
}
