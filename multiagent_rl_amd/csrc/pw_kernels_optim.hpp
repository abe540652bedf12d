// pw_kernels_optim.hpp -- part of libpworld.so (translation unit csrc/pworld_optim.hip includes it).
// The tail of a network's update as ONE launch: global-norm clip, Adam step and the Polyak update of the target network
// (torch.nn.utils.clip_grad_norm_, torch.optim.Adam.step, ddpg_gumbel_fix.py:36-47), and the Polyak update alone.
//
// Work assignment.  The tensor table (<= PW_OPT_MAX_TENSORS entries) travels in the kernarg segment.  Tensor k is cut into
// tiles of kOptTile elements; workgroup w serves tile w of the concatenated tile list (tile_begin[] is the host's prefix sum).
// Every access is one float per lane, lanes on consecutive addresses: a tensor may start at any 4-byte boundary and have any
// length, which is what nn.LSTM.flatten_parameters() produces (views into one flat buffer), so nothing here assumes 16-byte
// alignment.  At the sizes this serves (tens of thousands of elements) the launch is latency bound, not bandwidth bound.
//
// Global norm.  No workgroup waits for another: a workgroup that needs the norm computes it itself, from ALL gradients of
// the call (<= 2^20 floats, L2 hits after the first reader).  Lane l of the workgroup sums g^2 over elements l, l + 512, ...
// of tensor 0, then tensor 1, ... in float64 (g^2 is exact there), and the 512 partial sums are added pairwise through LDS,
// stride 256, 128, ... 1.  The order is fixed by the code and the same in every workgroup, so every workgroup holds the same
// bits: one coef for the whole call, identical from run to run; no atomics.  Against the exactly rounded result the float64
// sum is off by < 2^20 * 2^-53, so total_norm = (float)sqrt(sum) is within one float32 rounding of the true norm.
//   coef = (float)min(1, max_norm / (sqrt(sum) + 1e-6))            evaluated in float64, as clip_grad_norm_ states it
// A NaN among the gradients makes the sum, total_norm and coef NaN, and with them every element of a clipping call, exactly as
// clip_grad_norm_ multiplies every gradient by its NaN coefficient (min() written so that NaN passes: c >= 1 ? 1 : c).  An
// infinite norm gives coef = 0, as there.  A call that does not clip has no coef: a NaN stays in its own element.
// Gradients are READ ONLY: unlike clip_grad_norm_, which scales .grad in place, the scaled gradient exists in registers only.
//
// Adam, the float32 operation order of one element (-ffp-contract=off: only the fma written below fuses):
//   g  = grad * coef                              (skipped when the call does not clip)
//   g  = fma(wd, p, g)                            (weight_decay != 0: the L2 form, after the clip)
//   m  = fma(m, beta1, g * (1 - beta1))           (1 - beta1, 1 - beta2: float64 on the host, then rounded)
//   v  = fma(v, beta2, (g * g) * (1 - beta2))
//   d  = sqrt(v) / sqrt(1 - beta2^step) + eps     (IEEE sqrt and division; the bias corrections: float64 on the host --
//                                                   pw_adam_step_dev: float64 in the kernel, pw_optim_bias.hpp)
//   p  = fma(-(lr / (1 - beta1^step)), m / d, p)
// torch.optim.Adam(foreach=False) forms m with lerp and v with mul + addcmul: a different, equally long rounding chain.
//
// Soft update: t = t * (float)(1 - tau) + p * (float)tau, both products rounded before the sum -- bit for bit what torch
// computes for `t * (1.0 - tau) + p * tau` -- on the p this launch has just written.  tau == 1 stores p itself (hard_update):
// the old target is not read, so an infinity there cannot turn into NaN through inf * 0.
#pragma once

#include <hip/hip_runtime.h>

#include "pworld.h"
#include "pw_optim_args.hpp"

namespace {

// The body is text shared with pw_adam_step_dev_kernel (pw_kernels_optim_dev.hpp); the two scalars that kernel forms itself are macros here.
__global__ void __launch_bounds__(kOptThreads) pw_adam_step_kernel(const OptArgs A)
{
    __shared__ double s_part[kOptThreads];
#define PW_ADAM_BC2_SQRT A.bc2_sqrt
#define PW_ADAM_STEP_SIZE A.step_size
#include "pw_kernels_optim_adam_body.inc"
#undef PW_ADAM_BC2_SQRT
#undef PW_ADAM_STEP_SIZE
}

__global__ void __launch_bounds__(kOptThreads) pw_soft_update_kernel(const SoftArgs A)
{
    const int lane = threadIdx.x;
    const int k = opt_tile_owner(A, (int)blockIdx.x);
    const SoftTensor T = A.t[k];
    const long base = (long)((int)blockIdx.x - A.tile_begin[k]) * kOptTile;
#pragma unroll
    for (int j = 0; j < kOptTile / kOptThreads; ++j) {
        const long i = base + j * kOptThreads + lane;
        if (i >= T.numel) break;
        const float p = T.source[i];
        T.target[i] = A.hard ? p : opt_polyak(T.target[i], p, A.omt, A.tau);
    }
}

}  // namespace
