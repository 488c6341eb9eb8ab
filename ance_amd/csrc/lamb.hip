// Fused multi-tensor LAMB step (include/ance_amd.h: ance_lamb_step): the reference's utils/lamb.py Lamb.step -- a Python loop
// of ~19 small launches and up to three host synchronisations per parameter tensor -- as three launches for every tensor of the
// call and no host synchronisation.
//   pass 1   (one workgroup per 16,384-element chunk)  m, v updated; u = m / (sqrt(v) + eps) [+ wd p]; the chunk's sums of p^2
//            and u^2 (fp64) stored to its slot: reads p, g, m, v (16 B / element), writes m, v (8 B)
//   reduce   (one wave per tensor)  the tensor's chunk sums added in chunk order (fp64) -> wn, an, tr into d_out [t][3]
//   pass 2   (one workgroup per chunk)  u recomputed from p, m, v by the same code as pass 1; p += (-lr tr) u: reads 12 B, writes 4 B
// 40 B of HBM traffic per element.  No atomics and a fixed summation order everywhere: the same inputs give the same bits (under
// DDP every rank steps on the same all-reduced gradients and must stay bit-identical).  Division and sqrtf are the IEEE ones
// (hipcc's default correctly rounded fp32 divide / sqrt), as in the reference's fp32 arithmetic.
//
// ance_lamb_step_clipped: torch.nn.utils.clip_grad_norm_(params, max_grad_norm) (2-norm, error_if_nonfinite=False) fused in front,
// two more launches and 4 B more per element (44 B; clip_grad_norm_ then the step moves 52 B in a dozen launches):
//   gnorm    (one workgroup per chunk; multi_tensor.hip)  reads g only; the chunk's sum of g^2 (fp64) stored to its slot
//   gtotal   (one workgroup)  the chunk sums added in chunk order (fp64), one sqrt, rounded to fp32 -> *d_grad_norm;
//            coef = min(max_grad_norm / (total + 1e-6), 1) in fp32, NaN when the total is NaN (as torch's clamp)
//   pass 1   as above with g * coef (an fp32 product, formed in registers) in place of g; the gradients in memory are not rescaled
//
// ance_lamb_step_amp: either step under loss scaling (torch.amp.GradScaler's contract for optimizers that set
// _step_supports_amp_scaling: the scale and the overflow flag arrive as device scalars and step() is called unconditionally).  No
// launch more: three without clipping, five with it, and still no atomics, a fixed summation order and no host synchronisation.
//   unscale  d_grad_scale given: inv = (float)(1.0 / (double)*d_grad_scale), the value GradScaler.unscale_ forms; every workgroup
//            that reads gradients forms it from the one device scalar by the same correctly rounded fp64 divide, so it is one
//            value.  Every gradient element enters the step as the fp32 product g * inv, formed in registers: gnorm squares and
//            sums those products, pass 1 takes (g * inv) * coef -- two fp32 roundings in that order.  The gradients in memory are
//            not rewritten.  A power-of-two scale is bit-neutral against the plain step on the unscaled gradients.
//   skip     d_found_inf given and !(*d_found_inf == 0) (an overflow count or NaN): every workgroup of pass 1 and pass 2 reads the
//            flag and returns before any store, so no bit of p, m, v changes; gnorm and gtotal still run (*d_grad_norm is
//            written and may be inf or NaN); reduce writes the rows of d_prev_out (or (0, 0, 1)) into d_out instead of new norms
//            and one thread adds 1 to *d_skipped with an ordinary load, add and store.
// Without the two pointers the launches and the instantiations are those of ance_lamb_step / ance_lamb_step_clipped.
//
// ance_lamb_step_scaled: the planned step for a loss scaler that hands no flag in.  gnorm runs with and without the clip, and gtotal
// (lamb_gtotal_flag_kernel) stores the overflow flag from its fp64 total -- 1 when it is not finite -- before pass 1 reads it: five
// launches either way, and with a finite total the bits of the planned step with a flag of 0.
//
// Here: LAMB's arithmetic, pass 1, reduce, gtotal and pass 2, its group rows and its entry points.  The walk of a workgroup over its
// chunk, the block sum and the device tensor row are multi_tensor.h's; the checks and the fill of the tables, the staging pool and
// gnorm are multi_tensor.hip's, shared with adamw.hip.
#include "multi_tensor.h"

namespace ance {
namespace {

using mt::align16;
using mt::DevTensor;
constexpr int LAMB_THREADS = mt::THREADS;

struct LambDevGroup {
    float b1, omb1, b2, omb2, eps, wd, neg_lr;
    int32_t has_wd;
    const double *d_lr;  // the learning rate as a device fp64 scalar (a resident plan's group with a tensor lr), or null: neg_lr holds it
};

// -lr of a group as the fp32 the update multiplies by: the host double, or the device scalar, negated and rounded the same way
__device__ __forceinline__ float lamb_neg_lr(const LambDevGroup &G) { return G.d_lr ? (float)(-G.d_lr[0]) : G.neg_lr; }

__device__ __forceinline__ float lamb_u(float p, float m, float v, const LambDevGroup &G) {
    float u = m / (sqrtf(v) + G.eps);
    if (G.has_wd) u = __builtin_fmaf(G.wd, p, u);
    return u;
}

// m, v update of one element; returns u
__device__ __forceinline__ float lamb_mv(float p, float g, float &m, float &v, const LambDevGroup &G) {
    m = __builtin_fmaf(G.omb1, g, m * G.b1);
    v = __builtin_fmaf(G.omb2 * g, g, v * G.b2);
    return lamb_u(p, m, v, G);
}

// CLIP: every gradient element is multiplied by *coef (ance_lamb_step_clipped) before it enters m and v; UNSCALE: by the inverse
// of *grad_scale before that (ance_lamb_step_amp).  found_inf (nullable): a skipped step returns before any store.
template <bool CLIP, bool UNSCALE>
__global__ void __launch_bounds__(LAMB_THREADS) lamb_pass1_kernel(const LambDevGroup *groups, const DevTensor *tensors,
                                                                  const int32_t *chunk_tensor, double2 *partial, const float *coef,
                                                                  const float *grad_scale, const float *found_inf) {
    if (mt::skip(found_inf)) return;
    const float cf = CLIP ? coef[0] : 1.0f;
    const float inv = UNSCALE ? mt::inv_scale(grad_scale) : 1.0f;
    const DevTensor T = tensors[chunk_tensor[blockIdx.x]];
    const LambDevGroup G = groups[T.group];
    float *a[4];
    const int len = mt::chunk_of(T, a);
    double s[2] = {0.0, 0.0};  // of p^2, of u^2
    mt::stream_chunk<0b1111, 0b1100>(a, len, T.vec, [&](float(&x)[4]) {
        const float u = lamb_mv(x[0], mt::grad<CLIP, UNSCALE>(x[1], inv, cf), x[2], x[3], G);
        s[0] = __builtin_fma((double)x[0], (double)x[0], s[0]);
        s[1] = __builtin_fma((double)u, (double)u, s[1]);
    });
    if (mt::block_sum(s)) partial[blockIdx.x] = make_double2(s[0], s[1]);
}

// one workgroup: every chunk's sum in chunk order (thread-strided, then a shared-memory tree) -> the total norm and the clip factor
__global__ void __launch_bounds__(1024) lamb_gtotal_kernel(const double *gpartial, int n_chunks, float max_norm, float *grad_norm,
                                                           float *coef) {
    __shared__ double s[1024];
    mt::grad_total(gpartial, n_chunks, max_norm, grad_norm, coef, s);
}

// gtotal of ance_lamb_step_scaled: the same total, and the step's own overflow flag from it (multi_tensor.h: grad_total_flag).
// Without CLIP only the flag is written.
template <bool CLIP>
__global__ void __launch_bounds__(1024) lamb_gtotal_flag_kernel(const double *gpartial, int n_chunks, float max_norm, float *grad_norm,
                                                                float *coef, float *found_inf) {
    __shared__ double s[1024];
    mt::grad_total_flag<CLIP>(gpartial, n_chunks, max_norm, grad_norm, coef, found_inf, s);
}

// one wave per tensor: chunk sums in chunk order (lane-strided, then an xor-shuffle tree) -> (wn, an, tr).  A skipped step
// (found_inf) has no chunk sums: the tensor's row is the one of prev_out, or (0, 0, 1) without it, and one thread counts the skip.
__global__ void __launch_bounds__(256) lamb_reduce_kernel(const DevTensor *tensors, int n_tensors, const double2 *partial,
                                                          float *out, const float *found_inf, const float *prev_out,
                                                          int64_t *skipped) {
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6), l = threadIdx.x & 63;
    if (t >= n_tensors) return;
    if (mt::skip(found_inf)) {
        if (l == 0) {
            const float wn = prev_out ? prev_out[3 * (int64_t)t] : 0.0f, an = prev_out ? prev_out[3 * (int64_t)t + 1] : 0.0f;
            const float tr = prev_out ? prev_out[3 * (int64_t)t + 2] : 1.0f;
            out[3 * (int64_t)t] = wn;
            out[3 * (int64_t)t + 1] = an;
            out[3 * (int64_t)t + 2] = tr;
            if (t == 0 && skipped) skipped[0] = skipped[0] + 1;
        }
        return;
    }
    const int c0 = tensors[t].chunk0, nc = tensors[t].n_chunks;
    double sp = 0.0, su = 0.0;
    for (int c = l; c < nc; c += 64) {
        const double2 s = partial[c0 + c];
        sp += s.x;
        su += s.y;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        sp += __shfl_xor(sp, off);
        su += __shfl_xor(su, off);
    }
    if (l == 0) {
        float wn = (float)sqrt(sp);
        wn = wn > 10.0f ? 10.0f : wn;  // clamp(0, 10) that lets a NaN through, as torch's clamp does
        const float an = (float)sqrt(su);
        const float tr = (wn == 0.0f || an == 0.0f) ? 1.0f : wn / an;
        out[3 * (int64_t)t] = wn;
        out[3 * (int64_t)t + 1] = an;
        out[3 * (int64_t)t + 2] = tr;
    }
}

__global__ void __launch_bounds__(LAMB_THREADS) lamb_pass2_kernel(const LambDevGroup *groups, const DevTensor *tensors,
                                                                  const int32_t *chunk_tensor, const float *out, int adam,
                                                                  const float *found_inf) {
    if (mt::skip(found_inf)) return;
    const int t = chunk_tensor[blockIdx.x];
    const DevTensor T = tensors[t];
    const LambDevGroup G = groups[T.group];
    const float tr = adam ? 1.0f : out[3 * (int64_t)t + 2];
    const float s = lamb_neg_lr(G) * tr;  // the reference's -step_size * trust_ratio, an fp32 product
    float *a[4];
    const int len = mt::chunk_of(T, a);
    mt::stream_chunk<0b1101, 0b0001>(a, len, T.vec, [&](float(&x)[4]) { x[0] = __builtin_fmaf(s, lamb_u(x[0], x[2], x[3], G), x[0]); });
}

// workspace: [groups][tensors][chunk -> tensor] (staged from the host in one copy: multi_tensor.h) [fp64 (p^2, u^2) per chunk]
size_t workspace_bytes_for(int n_tensors, int n_groups, int64_t n_chunks) {
    return mt::staged(sizeof(LambDevGroup), n_tensors, n_groups, n_chunks).end + sizeof(double2) * (size_t)n_chunks;
}
// the clipped step appends [fp64 g^2 per chunk][coef (fp32, 16 bytes)]
size_t workspace_bytes_clipped(int n_tensors, int n_groups, int64_t n_chunks) {
    return workspace_bytes_for(n_tensors, n_groups, n_chunks) + align16(sizeof(double) * (size_t)n_chunks) + 16;
}

// the reference's Python doubles, rounded to fp32 as torch does for a scalar
void lamb_group_row(void *row, const AnceLambGroup &a, const double *d_lr) {
    LambDevGroup &G = *(LambDevGroup *)row;
    G.d_lr = d_lr;
    G.b1 = (float)a.beta1;
    G.omb1 = (float)(1.0 - a.beta1);
    G.b2 = (float)a.beta2;
    G.omb2 = (float)(1.0 - a.beta2);
    G.eps = (float)a.eps;
    G.wd = (float)a.weight_decay;
    G.neg_lr = (float)(-a.lr);
    G.has_wd = a.weight_decay != 0.0;
}

// what ance_lamb_step_amp adds to a step: every pointer nullable, all null for the other two entry points
struct LambAmp {
    const float *grad_scale = nullptr, *found_inf = nullptr, *prev_out = nullptr;
    int64_t *skipped = nullptr;
    float *flag_out = nullptr;  // ance_lamb_step_scaled: the step writes the flag itself (found_inf == flag_out) and always runs gnorm
};

template <bool CLIP, bool UNSCALE>
void launch_pass1(int64_t n_chunks, hipStream_t st, const LambDevGroup *dG, const DevTensor *dT, const int32_t *dC, double2 *dP,
                  const float *dCoef, const LambAmp &amp) {
    hipLaunchKernelGGL((lamb_pass1_kernel<CLIP, UNSCALE>), dim3((unsigned)n_chunks), dim3(LAMB_THREADS), 0, st, dG, dT, dC, dP, dCoef,
                       amp.grad_scale, amp.found_inf);
}

// the launches of a step whose tables stand at the head of ws (layout L): three, or five with the clip or with a flag of its own
int lamb_launch(const char *fn, int n_tensors, int64_t n_chunks, const mt::Staged &L, int adam, float *d_out, char *ws, hipStream_t st,
                bool clip, double max_norm, float *d_grad_norm, const LambAmp &amp) {
    const LambDevGroup *dG = (const LambDevGroup *)ws;
    const DevTensor *dT = (const DevTensor *)(ws + L.tensors);
    const int32_t *dC = (const int32_t *)(ws + L.chunk_tensor);
    double2 *dP = (double2 *)(ws + L.end);
    const bool unscale = amp.grad_scale != nullptr;
    // behind the chunk sums of pass 1, in the clipped layout only: never dereferenced by a step without clip and flag
    double *dGP = (double *)(ws + L.end + sizeof(double2) * (size_t)n_chunks);
    float *dCoef = (float *)((char *)dGP + align16(sizeof(double) * (size_t)n_chunks));
    if (clip || amp.flag_out) {
        mt::launch_gnorm(n_chunks, st, dT, dC, dGP, amp.grad_scale);
        if (!amp.flag_out)
            hipLaunchKernelGGL(lamb_gtotal_kernel, dim3(1), dim3(1024), 0, st, (const double *)dGP, (int)n_chunks, (float)max_norm,
                               d_grad_norm, dCoef);
        else if (clip)
            hipLaunchKernelGGL(lamb_gtotal_flag_kernel<true>, dim3(1), dim3(1024), 0, st, (const double *)dGP, (int)n_chunks,
                               (float)max_norm, d_grad_norm, dCoef, amp.flag_out);
        else
            hipLaunchKernelGGL(lamb_gtotal_flag_kernel<false>, dim3(1), dim3(1024), 0, st, (const double *)dGP, (int)n_chunks, 0.0f,
                               (float *)nullptr, (float *)nullptr, amp.flag_out);
    }
    if (clip) {
        if (n_chunks > 0) {
            if (unscale) launch_pass1<true, true>(n_chunks, st, dG, dT, dC, dP, dCoef, amp);
            else launch_pass1<true, false>(n_chunks, st, dG, dT, dC, dP, dCoef, amp);
        }
    } else if (n_chunks > 0) {
        if (unscale) launch_pass1<false, true>(n_chunks, st, dG, dT, dC, dP, nullptr, amp);
        else launch_pass1<false, false>(n_chunks, st, dG, dT, dC, dP, nullptr, amp);
    }
    hipLaunchKernelGGL(lamb_reduce_kernel, dim3((unsigned)((n_tensors + 3) / 4)), dim3(256), 0, st, dT, n_tensors,
                       (const double2 *)dP, d_out, amp.found_inf, amp.prev_out, amp.skipped);
    if (n_chunks > 0)
        hipLaunchKernelGGL(lamb_pass2_kernel, dim3((unsigned)n_chunks), dim3(LAMB_THREADS), 0, st, dG, dT, dC, (const float *)d_out,
                           adam ? 1 : 0, amp.found_inf);
    return check_launch(fn);
}

// the checks a plan makes of its tables; ANCE_OK with *n_chunks, or a refusal in fn's name
int lamb_check_tables(const char *fn, const AnceLambTensor *h_tensors, int n_tensors, const AnceLambGroup *h_groups, int n_groups,
                      int64_t *n_chunks) {
    if (!h_tensors || !h_groups) return refuse(fn, "null table");
    if (n_groups < 1) return refuse(fn, "n_groups < 1");
    return mt::count_chunks(fn, h_tensors, n_tensors, n_groups, n_chunks);
}

// the body of ance_lamb_step (clip false), ance_lamb_step_clipped (clip true: max_norm, d_grad_norm) and ance_lamb_step_amp (amp);
// fn: the entry point's name, for the error text
int lamb_step_impl(const char *fn, const AnceLambTensor *h_tensors, int n_tensors, const AnceLambGroup *h_groups, int n_groups, int adam,
                   float *d_out, void *d_workspace, size_t workspace_bytes, void *stream, bool clip, double max_norm,
                   float *d_grad_norm, const LambAmp &amp) {
    if (n_tensors < 0) return refuse(fn, "n_tensors < 0");
    if (n_tensors == 0) return ANCE_OK;
    if (!h_tensors || !h_groups) return refuse(fn, "null table");
    if (n_groups < 1) return refuse(fn, "n_groups < 1");
    if (!d_out) return refuse(fn, "null d_out");
    int64_t n_chunks = 0;
    if (const int e = mt::count_chunks(fn, h_tensors, n_tensors, n_groups, &n_chunks)) return e;
    const size_t need = clip ? workspace_bytes_clipped(n_tensors, n_groups, n_chunks) : workspace_bytes_for(n_tensors, n_groups, n_chunks);
    if (!d_workspace || (uintptr_t)d_workspace % 16) return refuse(fn, "null or unaligned workspace");
    if (workspace_bytes < need) return refuse(fn, "workspace too small");

    const mt::Staged L = mt::staged(sizeof(LambDevGroup), n_tensors, n_groups, n_chunks);
    hipStream_t st = (hipStream_t)stream;
    char *ws = (char *)d_workspace;
    if (const int e = mt::stage_tables(fn, h_tensors, n_tensors, h_groups, n_groups, sizeof(LambDevGroup), lamb_group_row, L, ws, st))
        return e;
    return lamb_launch(fn, n_tensors, n_chunks, L, adam, d_out, ws, st, clip, max_norm, d_grad_norm, amp);
}

}  // namespace
}  // namespace ance

extern "C" size_t ance_lamb_workspace_bytes(int n_tensors, int n_groups, int64_t total_numel) {
    using namespace ance;
    if (n_tensors < 0 || n_groups < 1 || total_numel < 0) return 0;
    const int64_t chunks = mt::max_chunks(n_tensors, total_numel);
    if (chunks > (int64_t)INT32_MAX) return 0;
    return workspace_bytes_for(n_tensors, n_groups, chunks);
}

extern "C" int ance_lamb_step(const AnceLambTensor *h_tensors, int n_tensors, const AnceLambGroup *h_groups, int n_groups, int adam,
                              float *d_out, void *d_workspace, size_t workspace_bytes, void *stream) {
    using namespace ance;
    return lamb_step_impl("ance_lamb_step", h_tensors, n_tensors, h_groups, n_groups, adam, d_out, d_workspace, workspace_bytes, stream, false, 0.0, nullptr, LambAmp());
}

extern "C" size_t ance_lamb_clipped_workspace_bytes(int n_tensors, int n_groups, int64_t total_numel) {
    using namespace ance;
    if (n_tensors < 0 || n_groups < 1 || total_numel < 0) return 0;
    const int64_t chunks = mt::max_chunks(n_tensors, total_numel);
    if (chunks > (int64_t)INT32_MAX) return 0;
    return workspace_bytes_clipped(n_tensors, n_groups, chunks);
}

extern "C" int ance_lamb_step_clipped(const AnceLambTensor *h_tensors, int n_tensors, const AnceLambGroup *h_groups, int n_groups,
                                      int adam, double max_grad_norm, float *d_grad_norm, float *d_out, void *d_workspace,
                                      size_t workspace_bytes, void *stream) {
    using namespace ance;
    const char *fn = "ance_lamb_step_clipped";
    if (!(max_grad_norm > 0.0) || !(max_grad_norm < (double)INFINITY)) return refuse(fn, "max_grad_norm not a positive finite number");
    if (n_tensors > 0 && !d_grad_norm) return refuse(fn, "null d_grad_norm");
    return lamb_step_impl(fn, h_tensors, n_tensors, h_groups, n_groups, adam, d_out, d_workspace, workspace_bytes, stream, true,
                          max_grad_norm, d_grad_norm, LambAmp());
}

extern "C" size_t ance_lamb_amp_workspace_bytes(int n_tensors, int n_groups, int64_t total_numel) {
    return ance_lamb_clipped_workspace_bytes(n_tensors, n_groups, total_numel);  // enough with and without clipping
}

extern "C" int ance_lamb_step_amp(const AnceLambTensor *h_tensors, int n_tensors, const AnceLambGroup *h_groups, int n_groups, int adam,
                                  double max_grad_norm, const float *d_grad_scale, const float *d_found_inf, const float *d_prev_out,
                                  float *d_grad_norm, int64_t *d_skipped, float *d_out, void *d_workspace, size_t workspace_bytes,
                                  void *stream) {
    using namespace ance;
    const char *fn = "ance_lamb_step_amp";
    if (!(max_grad_norm >= 0.0) || !(max_grad_norm < (double)INFINITY))
        return refuse(fn, "max_grad_norm not 0 or a positive finite number");
    const bool clip = max_grad_norm != 0.0;
    if (clip && n_tensors > 0 && !d_grad_norm) return refuse(fn, "null d_grad_norm");
    LambAmp amp;
    amp.grad_scale = d_grad_scale;
    amp.found_inf = d_found_inf;
    amp.prev_out = d_prev_out;
    amp.skipped = d_skipped;
    return lamb_step_impl(fn, h_tensors, n_tensors, h_groups, n_groups, adam, d_out, d_workspace, workspace_bytes, stream, clip,
                          max_grad_norm, d_grad_norm, amp);
}

// ---- the resident plan: the tables are built once on the host, uploaded by the caller to the head of a workspace the plan owns,
// and every later step only launches (include/ance_amd.h)
extern "C" size_t ance_lamb_plan_table_bytes(int n_tensors, int n_groups, int64_t total_numel) {
    using namespace ance;
    if (n_tensors < 0 || n_groups < 1 || total_numel < 0) return 0;
    const int64_t chunks = mt::max_chunks(n_tensors, total_numel);
    if (chunks > (int64_t)INT32_MAX) return 0;
    return mt::staged(sizeof(LambDevGroup), n_tensors, n_groups, chunks).end;
}

extern "C" int ance_lamb_plan_build(const AnceLambTensor *h_tensors, int n_tensors, const AnceLambGroup *h_groups,
                                    const double *const *d_lrs, int n_groups, void *h_tables, size_t h_tables_bytes,
                                    int64_t *n_chunks_out, size_t *table_bytes_out) {
    using namespace ance;
    const char *fn = "ance_lamb_plan_build";
    if (n_tensors < 1) return refuse(fn, "n_tensors < 1");
    int64_t n_chunks = 0;
    if (const int e = lamb_check_tables(fn, h_tensors, n_tensors, h_groups, n_groups, &n_chunks)) return e;
    if (!h_tables || !n_chunks_out || !table_bytes_out) return refuse(fn, "null pointer");
    const mt::Staged L = mt::staged(sizeof(LambDevGroup), n_tensors, n_groups, n_chunks);
    if (h_tables_bytes < L.end) return refuse(fn, "h_tables too small");
    mt::fill_tables(h_tensors, n_tensors, h_groups, d_lrs, n_groups, sizeof(LambDevGroup), lamb_group_row, L, (char *)h_tables);
    *n_chunks_out = n_chunks;
    *table_bytes_out = L.end;
    return ANCE_OK;
}

extern "C" int ance_lamb_step_planned(int n_tensors, int n_groups, int64_t n_chunks, int adam, double max_grad_norm,
                                      const float *d_grad_scale, const float *d_found_inf, const float *d_prev_out, float *d_grad_norm,
                                      int64_t *d_skipped, float *d_out, void *d_workspace, size_t workspace_bytes, void *stream) {
    using namespace ance;
    const char *fn = "ance_lamb_step_planned";
    if (n_tensors < 1 || n_groups < 1 || n_chunks < 0 || n_chunks > (int64_t)INT32_MAX) return refuse(fn, "table sizes out of range");
    if (!(max_grad_norm >= 0.0) || !(max_grad_norm < (double)INFINITY))
        return refuse(fn, "max_grad_norm not 0 or a positive finite number");
    const bool clip = max_grad_norm != 0.0;
    if (clip && !d_grad_norm) return refuse(fn, "null d_grad_norm");
    if (!d_out) return refuse(fn, "null d_out");
    const size_t need = clip ? workspace_bytes_clipped(n_tensors, n_groups, n_chunks) : workspace_bytes_for(n_tensors, n_groups, n_chunks);
    if (!d_workspace || (uintptr_t)d_workspace % 16) return refuse(fn, "null or unaligned workspace");
    if (workspace_bytes < need) return refuse(fn, "workspace too small");
    LambAmp amp;
    amp.grad_scale = d_grad_scale;
    amp.found_inf = d_found_inf;
    amp.prev_out = d_prev_out;
    amp.skipped = d_skipped;
    const mt::Staged L = mt::staged(sizeof(LambDevGroup), n_tensors, n_groups, n_chunks);
    return lamb_launch(fn, n_tensors, n_chunks, L, adam, d_out, (char *)d_workspace, (hipStream_t)stream, clip, max_grad_norm, d_grad_norm,
                       amp);
}

// ance_lamb_step_planned for a caller that has no overflow flag to hand in: the step derives it (include/ance_amd.h)
extern "C" int ance_lamb_step_scaled(int n_tensors, int n_groups, int64_t n_chunks, int adam, double max_grad_norm,
                                     const float *d_grad_scale, float *d_found_inf, const float *d_prev_out, float *d_grad_norm,
                                     int64_t *d_skipped, float *d_out, void *d_workspace, size_t workspace_bytes, void *stream) {
    using namespace ance;
    const char *fn = "ance_lamb_step_scaled";
    if (n_tensors < 1 || n_groups < 1 || n_chunks < 0 || n_chunks > (int64_t)INT32_MAX) return refuse(fn, "table sizes out of range");
    if (!(max_grad_norm >= 0.0) || !(max_grad_norm < (double)INFINITY))
        return refuse(fn, "max_grad_norm not 0 or a positive finite number");
    const bool clip = max_grad_norm != 0.0;
    if (clip && !d_grad_norm) return refuse(fn, "null d_grad_norm");
    if (!d_grad_scale) return refuse(fn, "null d_grad_scale");
    if (!d_found_inf) return refuse(fn, "null d_found_inf");
    if (!d_out) return refuse(fn, "null d_out");
    if (!d_workspace || (uintptr_t)d_workspace % 16) return refuse(fn, "null or unaligned workspace");
    if (workspace_bytes < workspace_bytes_clipped(n_tensors, n_groups, n_chunks)) return refuse(fn, "workspace too small");
    LambAmp amp;
    amp.grad_scale = d_grad_scale;
    amp.found_inf = d_found_inf;
    amp.flag_out = d_found_inf;
    amp.prev_out = d_prev_out;
    amp.skipped = d_skipped;
    const mt::Staged L = mt::staged(sizeof(LambDevGroup), n_tensors, n_groups, n_chunks);
    return lamb_launch(fn, n_tensors, n_chunks, L, adam, d_out, (char *)d_workspace, (hipStream_t)stream, clip, max_grad_norm, d_grad_norm,
                       amp);
}
