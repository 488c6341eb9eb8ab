// transformers' get_linear_schedule_with_warmup on the device (include/ance_amd.h: ance_linear_warmup_step): what the reference's
// scheduler.step() does after every optimizer step -- last_epoch += 1, lr_g = base_lr_g * lambda(last_epoch) -- as ONE launch on
// device scalars, so that a captured training step carries its own schedule and the fused optimizers read each group's lr from
// memory (lamb.hip, adamw.hip: the group row's d_lr).
//   lambda(n) = n / max(1, warm)                                   for n < warm
//             = max(0, (total - n) / max(1, total - warm))         otherwise
// in fp64, expression for expression what _get_linear_schedule_with_warmup_lr_lambda computes with Python floats: two int -> fp64
// conversions, one IEEE division, one max, and LambdaLR's one product with the base lr.
#include "common.h"

namespace ance {
namespace {

__global__ void __launch_bounds__(256) linear_warmup_step_kernel(int64_t *d_n, const double *base_lrs, double *lrs, int n_groups,
                                                                 int64_t warm, int64_t total) {
    const int64_t n = d_n[0] + 1;  // every thread reads the old count, then one stores the new one
    __syncthreads();
    if (threadIdx.x == 0) d_n[0] = n;
    double lambda;
    if (n < warm) {
        lambda = (double)n / (double)(warm > 1 ? warm : 1);
    } else {
        const int64_t span = total - warm;
        lambda = (double)(total - n) / (double)(span > 1 ? span : 1);
        lambda = lambda > 0.0 ? lambda : 0.0;
    }
    for (int g = threadIdx.x; g < n_groups; g += 256) lrs[g] = base_lrs[g] * lambda;
}

}  // namespace
}  // namespace ance

extern "C" int ance_linear_warmup_step(int64_t *d_n, const double *d_base_lrs, double *d_lrs, int n_groups, int64_t num_warmup_steps,
                                       int64_t num_training_steps, void *stream) {
    using namespace ance;
    const char *fn = "ance_linear_warmup_step";
    if (!d_n || !d_base_lrs || !d_lrs || (uintptr_t)d_n % 8 || (uintptr_t)d_base_lrs % 8 || (uintptr_t)d_lrs % 8 || n_groups < 1) {
        set_last_error("ance_linear_warmup_step: invalid argument (null or unaligned pointer, or n_groups < 1)");
        return ANCE_E_INVALID;
    }
    hipLaunchKernelGGL(linear_warmup_step_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, d_n, d_base_lrs, d_lrs, n_groups,
                       num_warmup_steps, num_training_steps);
    return check_launch(fn);
}
