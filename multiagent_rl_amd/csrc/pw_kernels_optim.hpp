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
//   d  = sqrt(v) / sqrt(1 - beta2^step) + eps     (IEEE sqrt and division; the bias corrections: float64 on the host)
//   p  = fma(-(lr / (1 - beta1^step)), m / d, p)
// torch.optim.Adam(foreach=False) forms m with lerp and v with mul + addcmul: a different, equally long rounding chain.
//
// Soft update: t = t * (float)(1 - tau) + p * (float)tau, both products rounded before the sum -- bit for bit what torch
// computes for `t * (1.0 - tau) + p * tau` -- on the p this launch has just written.  tau == 1 stores p itself (hard_update):
// the old target is not read, so an infinity there cannot turn into NaN through inf * 0.
#pragma once

#include <hip/hip_runtime.h>

#include "pworld.h"

namespace {

constexpr int kOptThreads = 512;
constexpr int kOptTile = 2048;   // elements per workgroup: 4 per lane

struct OptTensor {
    float *param;
    const float *grad;
    float *exp_avg, *exp_avg_sq;
    float *target;
    long numel;
};

struct OptArgs {
    OptTensor t[PW_OPT_MAX_TENSORS];
    int tile_begin[PW_OPT_MAX_TENSORS + 1];
    int count;
    int need_norm;        // max_norm > 0 or total_norm wanted
    double max_norm;      // <= 0: no clipping
    float wd, beta1, beta2, omb1, omb2, eps, bc2_sqrt, step_size;
    float tau, omt;       // (float)tau, (float)(1 - tau)
    int hard;             // tau == 1
    float *total_norm;
};

struct SoftTensor {
    float *target;
    const float *source;
    long numel;
};

struct SoftArgs {
    SoftTensor t[PW_OPT_MAX_TENSORS];
    int tile_begin[PW_OPT_MAX_TENSORS + 1];
    int count;
    float tau, omt;
    int hard;
};

// The tensor that owns tile w: tile_begin[k] <= w < tile_begin[k + 1] (a uniform scan of at most 32 entries).
template <typename Args>
__device__ __forceinline__ int opt_tile_owner(const Args &A, const int w)
{
    int k = 0;
    while (k + 1 < A.count && A.tile_begin[k + 1] <= w) ++k;
    return k;
}

__device__ __forceinline__ float opt_polyak(const float t, const float p, const float omt, const float tau)
{
    const float a = t * omt, b = p * tau;
    return a + b;
}

__global__ void __launch_bounds__(kOptThreads) pw_adam_step_kernel(const OptArgs A)
{
    __shared__ double s_part[kOptThreads];
    const int lane = threadIdx.x;
    float coef = 1.0f;
    if (A.need_norm) {
        double acc = 0.0;
        for (int k = 0; k < A.count; ++k) {
            const float *__restrict__ g = A.t[k].grad;
            const long n = A.t[k].numel;
            for (long i = lane; i < n; i += kOptThreads) {
                const double x = (double)g[i];
                acc += x * x;
            }
        }
        s_part[lane] = acc;
        __syncthreads();
        for (int s = kOptThreads / 2; s > 0; s >>= 1) {
            if (lane < s) s_part[lane] += s_part[lane + s];
            __syncthreads();
        }
        const double norm = sqrt(s_part[0]);
        if (A.max_norm > 0.0) {
            const double c = A.max_norm / (norm + 1e-6);
            coef = (float)(c >= 1.0 ? 1.0 : c);   // NaN passes, as torch's clamp(max=1) lets it
        }
        if (A.total_norm != nullptr && blockIdx.x == 0 && lane == 0) *A.total_norm = (float)norm;
    }
    const int k = opt_tile_owner(A, (int)blockIdx.x);
    const OptTensor T = A.t[k];
    const long base = (long)((int)blockIdx.x - A.tile_begin[k]) * kOptTile;
    const bool clip = A.max_norm > 0.0;
#pragma unroll
    for (int j = 0; j < kOptTile / kOptThreads; ++j) {
        const long i = base + j * kOptThreads + lane;
        if (i >= T.numel) break;
        float g = T.grad[i];
        float p = T.param[i];
        if (clip) g = g * coef;
        if (A.wd != 0.0f) g = __builtin_fmaf(A.wd, p, g);
        const float m = __builtin_fmaf(T.exp_avg[i], A.beta1, g * A.omb1);
        const float v = __builtin_fmaf(T.exp_avg_sq[i], A.beta2, (g * g) * A.omb2);
        const float d = sqrtf(v) / A.bc2_sqrt + A.eps;
        p = __builtin_fmaf(-A.step_size, m / d, p);
        T.exp_avg[i] = m;
        T.exp_avg_sq[i] = v;
        T.param[i] = p;
        if (T.target != nullptr) T.target[i] = A.hard ? p : opt_polyak(T.target[i], p, A.omt, A.tau);
    }
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
