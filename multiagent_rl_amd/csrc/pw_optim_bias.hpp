// pw_optim_bias.hpp -- Adam's two step-dependent scalars as one host / device function: pw_adam_step_dev forms them in the kernel
// from a step count that lives in device memory, and csrc/pworld_optim.hip exports the same function to the host as
// pw_adam_bias_scalars, so the rule is testable without a GPU.
//
//   beta^t by square-and-multiply, least significant bit of t first:  r = 1; x = beta; while t: if t & 1: r *= x; x *= x; t >>= 1
//   bc2_sqrt  = (float)sqrt(1 - beta2^t)          step_size = (float)(lr / (1 - beta1^t))            all in float64
// Only IEEE float64 multiplications, one subtraction, a correctly rounded sqrt and a correctly rounded division (compile without
// FMA contraction): the host and the device produce the same bits.  pw_adam_step forms beta^t with std::pow instead; after the
// rounding to float32 the two agree at every t in [1, 20000] for (beta1, beta2, lr) in {(0.9, 0.999, 1e-2), (0.9, 0.999, 1e-3),
// (0.8, 0.99, 3e-4)} (tests/test_update_graph_host.py walks them).  A step below 1 counts as 1.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PW_OPT_HD __host__ __device__ inline
#else
#include <math.h>
#define PW_OPT_HD inline
#endif

PW_OPT_HD double pw_pow_square_multiply(double x, int64_t t)
{
    double r = 1.0;
    while (t > 0) {
        if (t & 1) r *= x;
        x *= x;
        t >>= 1;
    }
    return r;
}

PW_OPT_HD void pw_adam_bias(int64_t step, const double lr, const double beta1, const double beta2, float *bc2_sqrt, float *step_size)
{
    if (step < 1) step = 1;
    const double bc1 = 1.0 - pw_pow_square_multiply(beta1, step), bc2 = 1.0 - pw_pow_square_multiply(beta2, step);
    *bc2_sqrt = (float)sqrt(bc2);
    *step_size = (float)(lr / bc1);
}
