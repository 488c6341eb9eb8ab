// What the fused multi-tensor optimizer steps share (lamb.hip, adamw.hip).  Device side, here: the chunking of every tensor of a
// call into 16,384-element pieces, the walk of one workgroup over one chunk with float4 accesses (stream_chunk), the fixed-order
// block sum, the gradient element as it enters a step under loss scaling and clipping, and the total of the gradient-norm pass.
// Host side, declared here and defined in multi_tensor.hip: the checks and the fill of the host tables, their pinned staging pool,
// and the gradient-norm pass itself.
#pragma once
#include "common.h"

#include <float.h>
#include <math.h>

namespace ance {
namespace mt {

constexpr int CHUNK = 16384;  // elements per chunk: 16 float4 per thread and array at 256 threads
constexpr int THREADS = 256;
constexpr int UNROLL = 4;     // float4 per array in flight per thread

// the tensors' pointers come from a table, so the compiler cannot see they are global: say so, for global_load / global_store
// instead of flat accesses
typedef __attribute__((address_space(1))) float gfloat;
typedef __attribute__((address_space(1))) f32x4 gf32x4;

// *grad_scale -> the factor that unscales a gradient: the fp64 reciprocal rounded to fp32, as GradScaler.unscale_ (hipcc emits the
// correctly rounded fp32 divide for it, which is the same value: a 53-bit quotient rounds to 24 bits without a double-rounding error)
__device__ __forceinline__ float inv_scale(const float *grad_scale) { return (float)(1.0 / (double)grad_scale[0]); }

// the overflow flag of a step under loss scaling: anything but 0 skips, NaN included
__device__ __forceinline__ bool skip(const float *found_inf) { return found_inf && !(found_inf[0] == 0.0f); }

// the gradient element as it enters the step: unscaled, then clipped, each an fp32 product of its own
template <bool CLIP, bool UNSCALE>
__device__ __forceinline__ float grad(float g, float inv, float cf) {
    if (UNSCALE) g = g * inv;
    if (CLIP) g = g * cf;
    return g;
}

// one row of a step's device table: a tensor of the call and its chunks [chunk0, chunk0 + n_chunks) of the launch grid
struct DevTensor {
    float *p;
    const float *g;
    float *m, *v;
    float *step;  // AdamW's device step count; null for LAMB
    int64_t numel;
    int32_t chunk0, n_chunks, group, vec;  // vec: p, g, m and v are all 16-byte aligned
};

// workgroup blockIdx.x's chunk of T: its start in (p, g, m, v) -> a; returns its length
__device__ __forceinline__ int chunk_of(const DevTensor &T, float *(&a)[4]) {
    const int64_t base = (int64_t)(blockIdx.x - T.chunk0) * CHUNK;
    a[0] = T.p + base;
    a[1] = const_cast<float *>(T.g) + base;
    a[2] = T.m + base;
    a[3] = T.v + base;
    return (int)min((int64_t)CHUNK, T.numel - base);
}

// One workgroup of THREADS streams one chunk of N arrays: f(x) sees one element of every array, x[n] that of a[n]; the arrays of
// LOAD (bit n: a[n]) are read before it and those of STORE written after it.  vec: float4 accesses, UNROLL per array in flight
// (chunk starts are multiples of 4 elements, so an aligned tensor's chunks are aligned), and a scalar tail; else the whole chunk
// goes through the scalar loop.
template <unsigned LOAD, unsigned STORE, int N, class F>
__device__ __forceinline__ void stream_chunk(float *const (&a)[N], int len, int vec, F f) {
    const int tid = threadIdx.x;
    int done = 0;
    if (vec) {
        const int n4 = len >> 2;
        for (int i0 = tid; i0 < n4; i0 += THREADS * UNROLL) {
            f32x4 X[UNROLL][N];
#pragma unroll
            for (int k = 0; k < UNROLL; ++k) {
                const int i = i0 + k * THREADS;
                if (i < n4) {
#pragma unroll
                    for (int n = 0; n < N; ++n)
                        if (LOAD >> n & 1) X[k][n] = ((const gf32x4 *)a[n])[i];
                }
            }
#pragma unroll
            for (int k = 0; k < UNROLL; ++k) {
                const int i = i0 + k * THREADS;
                if (i < n4) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        float x[N];
#pragma unroll
                        for (int n = 0; n < N; ++n) x[n] = (LOAD >> n & 1) ? X[k][n][j] : 0.0f;
                        f(x);
#pragma unroll
                        for (int n = 0; n < N; ++n)
                            if (STORE >> n & 1) X[k][n][j] = x[n];
                    }
#pragma unroll
                    for (int n = 0; n < N; ++n)
                        if (STORE >> n & 1) ((gf32x4 *)a[n])[i] = X[k][n];
                }
            }
        }
        done = n4 * 4;
    }
    for (int e = done + tid; e < len; e += THREADS) {
        float x[N];
#pragma unroll
        for (int n = 0; n < N; ++n) x[n] = (LOAD >> n & 1) ? ((const gfloat *)a[n])[e] : 0.0f;
        f(x);
#pragma unroll
        for (int n = 0; n < N; ++n)
            if (STORE >> n & 1) ((gfloat *)a[n])[e] = x[n];
    }
}

// fixed-order sum of K doubles per thread over a workgroup of THREADS: an xor-shuffle tree inside each wave, then the waves in
// order.  True for thread 0, whose s holds the sums.
template <int K>
__device__ __forceinline__ bool block_sum(double (&s)[K]) {
    __shared__ double red[THREADS / 64][K];
    const int tid = threadIdx.x;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
#pragma unroll
        for (int k = 0; k < K; ++k) s[k] += __shfl_xor(s[k], off);
    if ((tid & 63) == 0)
#pragma unroll
        for (int k = 0; k < K; ++k) red[tid >> 6][k] = s[k];
    __syncthreads();
    if (tid != 0) return false;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        s[k] = red[0][k];
#pragma unroll
        for (int w = 1; w < THREADS / 64; ++w) s[k] += red[w][k];
    }
    return true;
}

// every thread of ONE workgroup of 1024: every chunk's sum in chunk order (thread-strided, then a shared-memory tree) -> the total
// norm (*grad_norm, the norm before clipping) and the clip factor min(max_norm / (total + 1e-6), 1) in fp32.  s: 1024 doubles of
// shared memory.  Ends with the workgroup synchronised and *coef stored by thread 0.
__device__ __forceinline__ void grad_total(const double *gpartial, int n_chunks, float max_norm, float *grad_norm, float *coef,
                                           double *s) {
    const int tid = threadIdx.x;
    double acc = 0.0;
    for (int c = tid; c < n_chunks; c += 1024) acc += gpartial[c];
    s[tid] = acc;
    __syncthreads();
    for (int off = 512; off > 0; off >>= 1) {
        if (tid < off) s[tid] += s[tid + off];
        __syncthreads();
    }
    if (tid == 0) {
        const float total = (float)sqrt(s[0]);
        const float c = max_norm / (total + 1e-6f);
        grad_norm[0] = total;
        coef[0] = c > 1.0f ? 1.0f : c;  // clamp(max=1) that lets a NaN through, as torch's clamp does
    }
}

// grad_total for a step that finds its own overflow (ance_*_step_scaled): the same sum in the same order, and thread 0 stores
// *found_inf = 1 when the fp64 total is not finite, else 0 -- an ordinary store, the only write of the flag.  The total is a sum of
// squares of fp32 values in fp64 (each at most 1.2e77, at most 2^31 * 16,384 of them: far inside the fp64 range), so it is finite
// exactly when every squared product g * inv is.  CLIP: *grad_norm and *coef as grad_total forms them; else neither is touched.
// Returns, to every thread of the workgroup, whether the step is skipped; ends with the workgroup synchronised.
template <bool CLIP>
__device__ __forceinline__ bool grad_total_flag(const double *gpartial, int n_chunks, float max_norm, float *grad_norm, float *coef,
                                                float *found_inf, double *s) {
    const int tid = threadIdx.x;
    double acc = 0.0;
    for (int c = tid; c < n_chunks; c += 1024) acc += gpartial[c];
    s[tid] = acc;
    __syncthreads();
    for (int off = 512; off > 0; off >>= 1) {
        if (tid < off) s[tid] += s[tid + off];
        __syncthreads();
    }
    const double sum = s[0];
    const bool overflow = !(fabs(sum) <= DBL_MAX);  // inf or NaN
    if (tid == 0) {
        found_inf[0] = overflow ? 1.0f : 0.0f;
        if (CLIP) {
            const float total = (float)sqrt(sum);
            const float c = max_norm / (total + 1e-6f);
            grad_norm[0] = total;
            coef[0] = c > 1.0f ? 1.0f : c;
        }
    }
    return overflow;
}

// ---- host side (multi_tensor.hip) ----
inline size_t align16(size_t b) { return (b + 15) & ~(size_t)15; }

inline int64_t max_chunks(int n_tensors, int64_t total_numel) {  // >= the sum of every tensor's ceil(numel / chunk)
    return (int64_t)n_tensors + total_numel / CHUNK;
}

// every row of a host table checked (Host: AnceLambTensor or AnceAdamwTensor) and the chunks of the call counted -> *n_chunks;
// ANCE_OK or a refusal in fn's name
template <class Host>
int count_chunks(const char *fn, const Host *h_tensors, int n_tensors, int n_groups, int64_t *n_chunks);

// what a step stages from the host in one copy, at the start of its workspace: [group rows][DevTensor rows][chunk -> tensor];
// byte offsets, end: where the step's own arrays begin
struct Staged {
    size_t tensors, chunk_tensor, end;
};
inline Staged staged(size_t group_row_bytes, int n_tensors, int n_groups, int64_t n_chunks) {
    Staged L;
    L.tensors = align16(group_row_bytes * (size_t)n_groups);
    L.chunk_tensor = L.tensors + align16(sizeof(DevTensor) * (size_t)n_tensors);
    L.end = L.chunk_tensor + align16(sizeof(int32_t) * (size_t)n_chunks);
    return L;
}

// a group row's fill: the host hyper-parameters and d_lr, the group's learning rate as a DEVICE fp64 scalar (null: a.lr holds it)
typedef void (*GroupRowFn)(void *row, const AnceLambGroup &a, const double *d_lr);

// the three tables in the layout L at h (host memory of L.end bytes): group row i by group_row(row, h_groups[i], d_lrs ? d_lrs[i] :
// null), the DevTensor rows and the chunk map.  Pure host code: what a resident plan keeps and what stage_tables sends
template <class Host>
void fill_tables(const Host *h_tensors, int n_tensors, const AnceLambGroup *h_groups, const double *const *d_lrs, int n_groups,
                 size_t group_row_bytes, GroupRowFn group_row, const Staged &L, char *h);

// fill_tables in a pinned staging buffer of the shared pool, sent to d_workspace on st.  ANCE_OK or an error in fn's name.  Not
// capturable (the pool queries and waits for events and may allocate): a captured step goes through a resident plan instead
template <class Host>
int stage_tables(const char *fn, const Host *h_tensors, int n_tensors, const AnceLambGroup *h_groups, int n_groups,
                 size_t group_row_bytes, GroupRowFn group_row, const Staged &L, void *d_workspace, hipStream_t st);

// gnorm: one workgroup per chunk reads g only; the chunk's sum of g^2 in fp64 -> gpartial[chunk].  grad_scale (nullable): of
// (g * inv)^2, the fp32 product squared
void launch_gnorm(int64_t n_chunks, hipStream_t st, const DevTensor *tensors, const int32_t *chunk_tensor, double *gpartial,
                  const float *grad_scale);

}  // namespace mt
}  // namespace ance
