// pw_kernels_sample.hpp -- part of libpworld.so (translation unit csrc/pworld_sample.hip includes it).
// The learner's Gumbel-softmax sample WITH gradient (F.gumbel_softmax(logits, tau, hard) of ddpg_gumbel_fix.py:150 and :178):
// pw_gumbel_st_forward_kernel and pw_gumbel_st_backward_kernel, one launch each instead of the dozen elementwise kernels, the softmax,
// the max and the scatter of the stock expression forward and its softmax chain backward.
//
// Shape: logits [rows][n], 1 <= n <= 16.  Mapping, the same for both kernels: one THREAD per row, 256-thread workgroups, no LDS, no
// barrier.  A row lives in registers: the kernels are templates on NB = ceil(n / 4) (1 .. 4), every loop over the logits has the
// compile-time bound 4 NB and is unrolled, and a logit past n is masked (its value is -inf forward, 0 backward; nothing is loaded
// or stored for it) -- no register array is indexed at run time, so none goes to scratch.
//
// Noise: value (row r, logit o) = log(-log(u)), u from word (o & 3) of Philox4x32-10 block (o >> 2) with
//   counter = (r lo, r hi | tag(blk), step lo, step hi), key = seed, tag(blk) = ((blk & 1) << 31) | ((blk >> 1) << 30),
// the uniform by pw_gumbel_uniform and both logarithms __logf: the key and the operations of the actor heads' noise
// (pw_kernels_policy.hpp, pw_gumbel_noise4), restated here so that this unit includes no kernel header of the actor family.
// oracle/actor_oracle.py gumbel_noise() is the float64 restatement of both.  The perturbed logit is logit - noise.
//
// Summation order is fixed (o ascending from zero, no atomics, -ffp-contract=off): the same inputs give the same bits.
// Addresses: 4-byte loads and stores only; a row's n numbers are contiguous, rows are n floats apart.
#pragma once

#include "pw_common.hpp"

namespace {

constexpr int kSampleMaxLogits = 16;   // four Philox blocks: the tag has two bits
constexpr int kSampleThreads = 256;

// the four noise values of block `blk` of row `grow` (pw_gumbel_noise4's key and operations)
__device__ __forceinline__ void sample_noise4(const uint64_t seed, const uint64_t step, const long grow, const uint32_t blk, float (&nz)[4])
{
    const uint32_t tag = ((blk & 1u) << 31) | ((blk >> 1) << 30);
    uint32_t u[4];
    pw_philox4x32_10((uint32_t)grow, (uint32_t)((uint64_t)grow >> 32) | tag, (uint32_t)step, (uint32_t)(step >> 32),
                     (uint32_t)seed, (uint32_t)(seed >> 32), u);
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const float uo = pw_gumbel_uniform(u[w]);  // in (0, 1)
        nz[w] = __logf(-__logf(uo));
    }
}

// v = (logit - noise) / tau;  idx = first maximum of v;  soft = softmax(v), maximum subtracted;  y = hard ? (onehot(idx) - soft) + soft
// : soft (the value of torch's y_hard - y_soft.detach() + y_soft, evaluated left to right).  soft, idx, noise: optional outputs.
template <int NB>
__global__ void __launch_bounds__(kSampleThreads) pw_gumbel_st_forward_kernel(const float *__restrict__ logits, const long rows, const int n,
                                                                              const float tau, const int hard, const uint64_t seed,
                                                                              uint64_t step, const int64_t *__restrict__ step_dev,
                                                                              float *__restrict__ y, float *__restrict__ soft,
                                                                              int32_t *__restrict__ idx, float *__restrict__ noise)
{
    const long r = (long)blockIdx.x * kSampleThreads + threadIdx.x;
    if (r >= rows) return;
    if (step_dev) step += (uint64_t)*step_dev;
    const long base = r * n;
    float v[4 * NB];
#pragma unroll
    for (int blk = 0; blk < NB; ++blk) {
        float nz[4];
        sample_noise4(seed, step, r, (uint32_t)blk, nz);
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const int o = 4 * blk + w;
            if (o < n) {
                v[o] = (logits[base + o] - nz[w]) / tau;
                if (noise) noise[base + o] = nz[w];
            } else {
                v[o] = -INFINITY;
            }
        }
    }
    int best = 0;
    float m = v[0];
#pragma unroll
    for (int o = 1; o < 4 * NB; ++o)
        if (o < n && v[o] > m) { m = v[o]; best = o; }   // strictly greater: the first maximum stays
    float sum = 0.0f;
#pragma unroll
    for (int o = 0; o < 4 * NB; ++o) {
        v[o] = o < n ? expf(v[o] - m) : 0.0f;
        sum += v[o];
    }
#pragma unroll
    for (int o = 0; o < 4 * NB; ++o) {
        if (o < n) {
            const float s = v[o] / sum;
            if (soft) soft[base + o] = s;
            y[base + o] = hard ? ((o == best ? 1.0f : 0.0f) - s) + s : s;
        }
    }
    if (idx) idx[r] = best;
}

// dLogits_o = soft_o (dY_o - sum_k dY_k soft_k) / tau, k ascending: the gradient of the soft sample, which is also the hard one's.
template <int NB>
__global__ void __launch_bounds__(kSampleThreads) pw_gumbel_st_backward_kernel(const float *__restrict__ dY, const float *__restrict__ soft,
                                                                               const long rows, const int n, const float tau,
                                                                               float *__restrict__ dLogits)
{
    const long r = (long)blockIdx.x * kSampleThreads + threadIdx.x;
    if (r >= rows) return;
    const long base = r * n;
    float s[4 * NB], g[4 * NB];
#pragma unroll
    for (int o = 0; o < 4 * NB; ++o) {
        s[o] = o < n ? soft[base + o] : 0.0f;
        g[o] = o < n ? dY[base + o] : 0.0f;
    }
    float dot = 0.0f;
#pragma unroll
    for (int o = 0; o < 4 * NB; ++o) dot += g[o] * s[o];   // the masked terms add +0
#pragma unroll
    for (int o = 0; o < 4 * NB; ++o)
        if (o < n) dLogits[base + o] = s[o] * (g[o] - dot) / tau;
}

}  // namespace
