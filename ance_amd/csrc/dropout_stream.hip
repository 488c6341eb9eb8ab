// The device dropout stream's one mutation (include/ance_amd.h: ance_dropout_stream_advance): base += n, enqueued once per training
// step behind the backward, so that a captured step draws the next step's masks at its next replay.  The kernels that read the
// stream are the dropout kernels themselves (philox.h: drop_stream).
#include "common.h"
#include "philox.h"

namespace ance {
namespace {

// one thread: an ordinary 64-bit load, add and store
__global__ void __launch_bounds__(64) dropout_stream_advance_kernel(uint64_t *d_stream, uint64_t n) {
    if (threadIdx.x == 0 && blockIdx.x == 0) d_stream[1] = d_stream[1] + n;
}

}  // namespace
}  // namespace ance

extern "C" int ance_dropout_stream_advance(uint64_t *d_stream, uint64_t n, void *stream) {
    using namespace ance;
    const char *fn = "ance_dropout_stream_advance";
    if (!d_stream || !stream_aligned(d_stream)) {
        set_last_error("ance_dropout_stream_advance: invalid argument (d_stream null or not 16-byte aligned)");
        return ANCE_E_INVALID;
    }
    if (n == 0) return ANCE_OK;
    hipLaunchKernelGGL(dropout_stream_advance_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, d_stream, n);
    return check_launch(fn);
}
