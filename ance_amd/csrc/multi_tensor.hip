// The host side of what the fused multi-tensor optimizer steps share (multi_tensor.h; lamb.hip, adamw.hip): the checks of a host
// table and its chunk count, the fill of the device tables (into a resident plan's own buffer, or into a pinned staging buffer of
// the pool here with their one copy to the workspace), the pool of those buffers, and the gradient-norm pass in front of a clipped
// step.
#include "multi_tensor.h"

#include <mutex>
#include <type_traits>
#include <vector>

namespace ance {
namespace mt {
namespace {

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
std::mutex g_stage_mu;
std::vector<Staging> g_stage;
unsigned long long g_stage_clock = 0;
long long g_stage_sends = 0;  // copies sent from the pool since the library was loaded (ance_debug_staging_sends)

// under g_stage_mu; returns the index of a buffer of >= bytes whose previous copy has run, or -1 (out of memory)
int stage_acquire(size_t bytes) {
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
int stage_send(Staging &S, void *d_dst, size_t bytes, hipStream_t st) {
    if (hipMemcpyAsync(d_dst, S.h, bytes, hipMemcpyHostToDevice, st) != hipSuccess) return 1;
    if (hipEventRecord(S.ev, st) != hipSuccess) return 2;
    S.recorded = true;
    S.last_use = ++g_stage_clock;
    ++g_stage_sends;
    return 0;
}

float *step_of(const AnceLambTensor &) { return nullptr; }
float *step_of(const AnceAdamwTensor &a) { return a.step; }

template <bool UNSCALE>
__global__ void __launch_bounds__(THREADS) gnorm_kernel(const DevTensor *tensors, const int32_t *chunk_tensor, double *gpartial,
                                                        const float *grad_scale) {
    const float inv = UNSCALE ? inv_scale(grad_scale) : 1.0f;
    const DevTensor T = tensors[chunk_tensor[blockIdx.x]];
    float *a[4];
    const int len = chunk_of(T, a);
    double sg[1] = {0.0};
    stream_chunk<0b0010, 0>(a, len, T.vec, [&](float(&x)[4]) {
        const double g = (double)grad<false, UNSCALE>(x[1], inv, 1.0f);
        sg[0] = __builtin_fma(g, g, sg[0]);
    });
    if (block_sum(sg)) gpartial[blockIdx.x] = sg[0];
}

}  // namespace


template <class Host>
int count_chunks(const char *fn, const Host *h_tensors, int n_tensors, int n_groups, int64_t *n_chunks) {
    int64_t n = 0;
    for (int t = 0; t < n_tensors; ++t) {
        const Host &T = h_tensors[t];
        if (T.group < 0 || T.group >= n_groups) return refuse(fn, "group index out of range");
        if (T.numel < 0) return refuse(fn, "numel < 0");
        if (T.numel > 0 && (!T.p || !T.g || !T.m || !T.v)) return refuse(fn, "null tensor pointer");
        if (std::is_same<Host, AnceAdamwTensor>::value && T.numel > 0 && !step_of(T))
            return refuse(fn, "null step of a tensor with elements");
        n += (T.numel + CHUNK - 1) / CHUNK;
        if (n > (int64_t)INT32_MAX) return refuse(fn, "too many elements");
    }
    *n_chunks = n;
    return ANCE_OK;
}

template <class Host>
void fill_tables(const Host *h_tensors, int n_tensors, const AnceLambGroup *h_groups, const double *const *d_lrs, int n_groups,
                 size_t group_row_bytes, GroupRowFn group_row, const Staged &L, char *h) {
    for (int i = 0; i < n_groups; ++i) group_row(h + group_row_bytes * (size_t)i, h_groups[i], d_lrs ? d_lrs[i] : nullptr);
    DevTensor *T = (DevTensor *)(h + L.tensors);
    int32_t *ct = (int32_t *)(h + L.chunk_tensor);
    int32_t c = 0;
    for (int t = 0; t < n_tensors; ++t) {
        const Host &a = h_tensors[t];
        T[t].p = a.p;
        T[t].g = a.g;
        T[t].m = a.m;
        T[t].v = a.v;
        T[t].step = step_of(a);
        T[t].numel = a.numel;
        T[t].group = a.group;
        T[t].chunk0 = c;
        T[t].n_chunks = (int32_t)((a.numel + CHUNK - 1) / CHUNK);
        T[t].vec = ((uintptr_t)a.p | (uintptr_t)a.g | (uintptr_t)a.m | (uintptr_t)a.v) % 16 == 0;
        for (int32_t k = 0; k < T[t].n_chunks; ++k) ct[c++] = t;
    }
}

template <class Host>
int stage_tables(const char *fn, const Host *h_tensors, int n_tensors, const AnceLambGroup *h_groups, int n_groups,
                 size_t group_row_bytes, GroupRowFn group_row, const Staged &L, void *d_workspace, hipStream_t st) {
    char what[96];
    std::lock_guard<std::mutex> lock(g_stage_mu);
    const int si = stage_acquire(L.end);
    if (si < 0) {
        snprintf(what, sizeof(what), "%s: pinned staging buffer", fn);
        set_last_error(what);
        return ANCE_E_NOMEM;
    }
    Staging &S = g_stage[si];
    fill_tables(h_tensors, n_tensors, h_groups, nullptr, n_groups, group_row_bytes, group_row, L, (char *)S.h);
    const int sent = stage_send(S, d_workspace, L.end, st);
    if (!sent) return ANCE_OK;
    snprintf(what, sizeof(what), sent == 1 ? "%s: tables" : "%s: staging event", fn);
    return check_launch(what);
}

template int count_chunks(const char *, const AnceLambTensor *, int, int, int64_t *);
template int count_chunks(const char *, const AnceAdamwTensor *, int, int, int64_t *);
template void fill_tables(const AnceLambTensor *, int, const AnceLambGroup *, const double *const *, int, size_t, GroupRowFn,
                          const Staged &, char *);
template void fill_tables(const AnceAdamwTensor *, int, const AnceLambGroup *, const double *const *, int, size_t, GroupRowFn,
                          const Staged &, char *);
template int stage_tables(const char *, const AnceLambTensor *, int, const AnceLambGroup *, int, size_t, GroupRowFn, const Staged &,
                          void *, hipStream_t);
template int stage_tables(const char *, const AnceAdamwTensor *, int, const AnceLambGroup *, int, size_t, GroupRowFn, const Staged &,
                          void *, hipStream_t);

void launch_gnorm(int64_t n_chunks, hipStream_t st, const DevTensor *tensors, const int32_t *chunk_tensor, double *gpartial,
                  const float *grad_scale) {
    if (n_chunks == 0) return;
    if (grad_scale)
        hipLaunchKernelGGL(gnorm_kernel<true>, dim3((unsigned)n_chunks), dim3(THREADS), 0, st, tensors, chunk_tensor, gpartial, grad_scale);
    else
        hipLaunchKernelGGL(gnorm_kernel<false>, dim3((unsigned)n_chunks), dim3(THREADS), 0, st, tensors, chunk_tensor, gpartial, grad_scale);
}

}  // namespace mt
}  // namespace ance

// how many table uploads have gone through the shared staging pool: a step through a resident plan adds none
extern "C" long long ance_debug_staging_sends(void) {
    std::lock_guard<std::mutex> lock(ance::mt::g_stage_mu);
    return ance::mt::g_stage_sends;
}
