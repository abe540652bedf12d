// pw_kernels_optim_dev.hpp -- part of libpworld.so (translation unit csrc/pworld_optim_dev.hip includes it).
// pw_adam_step (pw_kernels_optim.hpp states the arithmetic) with the step count in device memory: what a captured update launches.
#pragma once

#include "pw_optim_args.hpp"
#include "pw_optim_bias.hpp"

namespace {

// pw_adam_step with the step count in device memory (a captured launch freezes by-value arguments): every lane forms the two
// step-dependent scalars itself (pw_optim_bias.hpp: at most 2 x 63 float64 multiplications, one sqrt, one division -- uniform over the
// launch), then the same body.  The body is shared as text: as a __forceinline__ function called from both kernels it compiles
// pw_adam_step_kernel to other instructions than the body in the kernel does (other scalar loads of the argument block, other register
// numbers), and tools/code_object.py --compare holds every existing kernel to its parent's disassembly.
__global__ void __launch_bounds__(kOptThreads) pw_adam_step_dev_kernel(const OptArgs A, const int64_t *__restrict__ step_dev, const double lr,
                                                                       const double beta1, const double beta2)
{
    __shared__ double s_part[kOptThreads];
    float bc2_sqrt, step_size;
    pw_adam_bias(*step_dev, lr, beta1, beta2, &bc2_sqrt, &step_size);
#define PW_ADAM_BC2_SQRT bc2_sqrt
#define PW_ADAM_STEP_SIZE step_size
#include "pw_kernels_optim_adam_body.inc"
#undef PW_ADAM_BC2_SQRT
#undef PW_ADAM_STEP_SIZE
}

}  // namespace
