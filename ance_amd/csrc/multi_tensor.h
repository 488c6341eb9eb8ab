// What the fused multi-tensor optimizer steps share (lamb.hip, adamw.hip): the chunking of every tensor of a call into
// 16,384-element pieces that one workgroup each streams with float4 accesses, the gradient element as it enters a step under loss
// scaling and clipping, the gradient-norm pass and its fixed-order total, and the pinned staging pool of the host tables.
#pragma once
#include "common.h"

#include <math.h>
#include <mutex>
#include <vector>

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

// the chunk's sum of g^2 in fp64: reads g only.  UNSCALE: of (g * inv)^2, the fp32 product squared.  Tensor: a device table row
// with g, numel and chunk0 (each step has its own, so the instantiations of two source files never share a name)
template <class Tensor, bool UNSCALE>
__global__ void __launch_bounds__(THREADS) gnorm_kernel(const Tensor *tensors, const int32_t *chunk_tensor, double *gpartial,
                                                        const float *grad_scale) {
    __shared__ double red[THREADS / 64];
    const int tid = threadIdx.x;
    const float inv = UNSCALE ? inv_scale(grad_scale) : 1.0f;
    const Tensor T = tensors[chunk_tensor[blockIdx.x]];
    const int64_t base = (int64_t)(blockIdx.x - T.chunk0) * CHUNK;
    const int len = (int)min((int64_t)CHUNK, T.numel - base);
    const gfloat *g = (const gfloat *)(T.g + base);
    double sg = 0.0;
    int done = 0;
    if (T.vec) {
        const int n4 = len >> 2;
        const gf32x4 *g4 = (const gf32x4 *)g;
        for (int i0 = tid; i0 < n4; i0 += THREADS * UNROLL) {
            f32x4 Gr[UNROLL];
#pragma unroll
            for (int k = 0; k < UNROLL; ++k) {
                const int i = i0 + k * THREADS;
                Gr[k] = i < n4 ? g4[i] : f32x4{0.f, 0.f, 0.f, 0.f};
            }
#pragma unroll
            for (int k = 0; k < UNROLL; ++k)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const double x = (double)grad<false, UNSCALE>(Gr[k][j], inv, 1.0f);
                    sg = __builtin_fma(x, x, sg);
                }
        }
        done = n4 * 4;
    }
    for (int e = done + tid; e < len; e += THREADS) {
        const double x = (double)grad<false, UNSCALE>(g[e], inv, 1.0f);
        sg = __builtin_fma(x, x, sg);
    }
    // fixed-order block sum: xor-shuffle tree inside each wave, then the four waves in order
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sg += __shfl_xor(sg, off);
    if ((tid & 63) == 0) red[tid >> 6] = sg;
    __syncthreads();
    if (tid == 0) {
        double a = red[0];
#pragma unroll
        for (int w = 1; w < THREADS / 64; ++w) a += red[w];
        gpartial[blockIdx.x] = a;
    }
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

inline size_t align16(size_t b) { return (b + 15) & ~(size_t)15; }

inline int64_t max_chunks(int n_tensors, int64_t total_numel) {  // >= the sum of every tensor's ceil(numel / chunk)
    return (int64_t)n_tensors + total_numel / CHUNK;
}

// Pinned staging buffers of the host tables, one pool for every step of the library.  A buffer is handed out again only once the
// event recorded after its last copy has completed (hipEventQuery, no wait), so a pending DMA never reads a buffer that is being
// refilled.  When all of them are still in flight the pool grows; at its cap the caller waits for the oldest copy -- a host wait on
// a copy enqueued POOL steps ago.
constexpr int POOL = 16;
struct Staging {
    void *h = nullptr;
    size_t bytes = 0;
    hipEvent_t ev = nullptr;
    bool recorded = false;
    unsigned long long last_use = 0;
};
// one definition for every source file of the library (C++17 inline variables), hidden: the library exports its C ABI only
#define ANCE_MT_SHARED inline __attribute__((visibility("hidden")))
ANCE_MT_SHARED std::mutex g_stage_mu;
ANCE_MT_SHARED std::vector<Staging> g_stage;
ANCE_MT_SHARED unsigned long long g_stage_clock = 0;
#undef ANCE_MT_SHARED

// under g_stage_mu; returns the index of a buffer of >= bytes whose previous copy has run, or -1 (out of memory)
inline int stage_acquire(size_t bytes) {
    for (size_t i = 0; i < g_stage.size(); ++i) {
        Staging &s = g_stage[i];
        if (s.bytes >= bytes && (!s.recorded || hipEventQuery(s.ev) == hipSuccess)) return (int)i;
    }
    size_t want = 65536;
    while (want < bytes) want <<= 1;
    if ((int)g_stage.size() < POOL) {
        Staging s;
        if (hipHostMalloc(&s.h, want, hipHostMallocDefault) != hipSuccess) return -1;
        if (hipEventCreateWithFlags(&s.ev, hipEventDisableTiming) != hipSuccess) return -1;
        s.bytes = want;
        g_stage.push_back(s);
        return (int)g_stage.size() - 1;
    }
    int old = 0;
    for (int i = 1; i < (int)g_stage.size(); ++i)
        if (g_stage[i].last_use < g_stage[old].last_use) old = i;
    Staging &s = g_stage[old];
    if (s.recorded && hipEventSynchronize(s.ev) != hipSuccess) return -1;
    if (s.bytes < bytes) {  // the old buffer stays allocated: freeing pinned memory can synchronise the device
        void *h = nullptr;
        if (hipHostMalloc(&h, want, hipHostMallocDefault) != hipSuccess) return -1;
        s.h = h;
        s.bytes = want;
    }
    s.recorded = false;
    return old;
}

// under g_stage_mu: the first `bytes` of buffer S to the device on st, and the event that frees the buffer for its next use.
// Returns 0, 1 (the copy failed) or 2 (the event)
inline int stage_send(Staging &S, void *d_dst, size_t bytes, hipStream_t st) {
    if (hipMemcpyAsync(d_dst, S.h, bytes, hipMemcpyHostToDevice, st) != hipSuccess) return 1;
    if (hipEventRecord(S.ev, st) != hipSuccess) return 2;
    S.recorded = true;
    S.last_use = ++g_stage_clock;
    return 0;
}

}  // namespace mt
}  // namespace ance
