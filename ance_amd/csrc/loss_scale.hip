// The dynamic loss scale's update on the device (include/ance_amd.h: ance_loss_scale_update): what torch.amp.GradScaler.update()
// does through torch._amp_update_scale_, as ONE launch of one thread on three device scalars, so that a captured training step
// carries its scaler.  The arithmetic is that op's, roundings included:
//   flag != 0 (NaN included)   scale <- float32(float64(scale) * backoff_factor); tracker <- 0
//   else                       n = tracker + 1; n == growth_interval: s = float32(float64(scale) * growth_factor), scale <- s only
//                              if s is finite, tracker <- 0; otherwise tracker <- n
// The flag is the one a step of ance_*_step_scaled left (or any GradScaler-style overflow count).
#include "common.h"

#include <math.h>

namespace ance {
namespace {

__global__ void __launch_bounds__(1) loss_scale_update_kernel(float *scale, int32_t *tracker, const float *found_inf, double growth,
                                                               double backoff, int32_t interval) {
    if (!(found_inf[0] == 0.0f)) {
        scale[0] = (float)((double)scale[0] * backoff);
        tracker[0] = 0;
        return;
    }
    const int32_t n = tracker[0] + 1;
    if (n == interval) {
        const float grown = (float)((double)scale[0] * growth);
        if (fabsf(grown) <= 3.402823466e+38f) scale[0] = grown;  // never grown past the fp32 range to inf
        tracker[0] = 0;
    } else {
        tracker[0] = n;
    }
}

}  // namespace
}  // namespace ance

extern "C" int ance_loss_scale_update(float *d_scale, int32_t *d_growth_tracker, const float *d_found_inf, double growth_factor,
                                      double backoff_factor, int32_t growth_interval, void *stream) {
    using namespace ance;
    const char *fn = "ance_loss_scale_update";
    if (!d_scale || !d_growth_tracker || !d_found_inf) return refuse(fn, "null pointer");
    if ((uintptr_t)d_scale % 4 || (uintptr_t)d_growth_tracker % 4 || (uintptr_t)d_found_inf % 4) return refuse(fn, "unaligned pointer");
    if (!(growth_factor > 0.0) || !(growth_factor < (double)INFINITY)) return refuse(fn, "growth_factor not a positive finite number");
    if (!(backoff_factor > 0.0) || !(backoff_factor < (double)INFINITY)) return refuse(fn, "backoff_factor not a positive finite number");
    if (growth_interval < 1) return refuse(fn, "growth_interval < 1");
    hipLaunchKernelGGL(loss_scale_update_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, d_scale, d_growth_tracker, d_found_inf,
                       growth_factor, backoff_factor, growth_interval);
    return check_launch(fn);
}
