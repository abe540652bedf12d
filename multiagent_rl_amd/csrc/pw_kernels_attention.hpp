// pw_kernels_attention.hpp -- part of libpworld.so (translation unit csrc/pworld_attention.hip includes it).
// The attention block of CriticNetwork WITH gradient (critic.py: score of every LSTM step against the last one, softmax over the
// agent axis, weighted sum, ReLU), for the learner's two critic passes per update: pw_attention_pool_forward_kernel and
// pw_attention_pool_backward_kernel, one launch each instead of bmm / softmax / bmm / relu and their dozen backward kernels.  No parameters:
// dense1, the LSTM and dense2 stay where they are (torch GEMMs, csrc/pw_kernels_lstm.hpp).
//
// Shape: Y [b][N][64], 1 <= N <= 64.  Mapping, the same for both kernels:
//   * one WAVE per batch row, lane = hidden unit j: every load and store of a step is one contiguous 256-byte row, a score is a
//     wave reduction, and no LDS allocation, no barrier and no hand-off between waves exists (a workgroup is four independent rows);
//   * N <= 64 = the wave's width, so the per-step scalars (s_t, w_t, dw_t, ds_t) live in LANE t of one register: the softmax is two
//     more wave reductions over lanes < N, and the second pass fetches step t's scalar with v_readlane (t is wave-uniform).  No
//     per-step register array exists, so a run-time N indexes nothing;
//   * Y is read twice (score pass, then context / gradient pass): a row's tile is N x 256 B <= 16 KiB, the second read hits the
//     cache, and both passes issue their loads ahead of the reductions that consume them.
// Summation order is fixed (no atomics): a wave reduction is the butterfly lane ^ 1, 2, 4, 8, 16, 32 -- both partners add the same
// two numbers, so every lane ends with the same bits -- and the sums over t run t ascending as chains of fused multiply-adds
// from zero.  Two runs, another stream, weight stored or not: the same bits.
// Addresses: 4-byte loads and stores only (Y is a view of whatever produced it): every pointer 4-byte aligned.
// A workgroup's waves past the last row compute on row 0 and store nothing.
#pragma once

#include "pw_common.hpp"
#include "pw_lstm_math.hpp"

namespace {

constexpr int kAttnH = 64;          // hidden units = lanes of a wave
constexpr int kAttnMaxSteps = 64;   // one lane per step; pw_critic_forward's agent-axis bound
constexpr int kAttnThreads = 256;   // four rows per workgroup

__device__ __forceinline__ float attn_wave_sum(float v)
{
    v += __shfl_xor(v, 1); v += __shfl_xor(v, 2); v += __shfl_xor(v, 4); v += __shfl_xor(v, 8);
    v += lane_xor16(v); v += lane_xor32(v);
    return v;
}
__device__ __forceinline__ float attn_wave_max(float v)
{
    v = fmaxf(v, __shfl_xor(v, 1)); v = fmaxf(v, __shfl_xor(v, 2)); v = fmaxf(v, __shfl_xor(v, 4)); v = fmaxf(v, __shfl_xor(v, 8));
    v = fmaxf(v, lane_xor16(v)); v = fmaxf(v, lane_xor32(v));
    return v;
}
__device__ __forceinline__ float attn_lane_value(const float v, const int t)   // lane t's v, t wave-uniform
{
    return __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(v), t));
}

// <Y_t, x> for every t into lane t (0 where lane >= N); x is a per-lane (hidden unit) value
__device__ __forceinline__ float attn_dots(const float *__restrict__ y, const int N, const int j, const float x)
{
    float mine = 0.0f;
    float nxt = y[j];
    for (int t = 0; t < N; ++t) {
        const float cur = nxt;
        if (t + 1 < N) nxt = y[(t + 1) * kAttnH + j];   // the next row travels under this row's reduction
        const float s = attn_wave_sum(cur * x);
        if (j == t) mine = s;
    }
    return mine;
}

// Y [b][N][64] -> out [b][64], weight [b][N] or NULL
__global__ void __launch_bounds__(kAttnThreads) pw_attention_pool_forward_kernel(const float *__restrict__ Y, const long b, const int N,
                                                                                 const int relu, float *__restrict__ out,
                                                                                 float *__restrict__ weight)
{
    const int j = threadIdx.x % kAttnH;
    const long row = (long)blockIdx.x * (kAttnThreads / kAttnH) + threadIdx.x / kAttnH;
    const bool valid = row < b;
    const float *y = Y + (valid ? (size_t)row : 0) * N * kAttnH;
    const float q = y[(N - 1) * kAttnH + j];
    const float s = attn_dots(y, N, j, q);
    const bool step = j < N;
    const float mx = attn_wave_max(step ? s : -INFINITY);
    const float e = step ? expf(s - mx) : 0.0f;
    const float w = e / attn_wave_sum(e);
    float c = 0.0f;
    for (int t = 0; t < N; ++t) c = fmaf(attn_lane_value(w, t), y[t * kAttnH + j], c);
    if (valid) {
        out[(size_t)row * kAttnH + j] = relu ? relu_fwd(c) : c;
        if (weight && step) weight[(size_t)row * N + j] = w;
    }
}

// dOut [b][64], Y, weight and out as the forward read and wrote them -> dY [b][N][64]
__global__ void __launch_bounds__(kAttnThreads) pw_attention_pool_backward_kernel(const float *__restrict__ dOut, const float *__restrict__ Y,
                                                                                  const float *__restrict__ weight,
                                                                                  const float *__restrict__ out, const long b, const int N,
                                                                                  const int relu, float *__restrict__ dY)
{
    const int j = threadIdx.x % kAttnH;
    const long row = (long)blockIdx.x * (kAttnThreads / kAttnH) + threadIdx.x / kAttnH;
    const bool valid = row < b;
    const size_t r = valid ? (size_t)row : 0;
    const float *y = Y + r * N * kAttnH;
    const float q = y[(N - 1) * kAttnH + j];
    float dc = dOut[r * kAttnH + j];
    if (relu && !(out[r * kAttnH + j] > 0.0f)) dc = 0.0f;
    const float w = j < N ? weight[r * N + j] : 0.0f;
    const float dw = attn_dots(y, N, j, dc);
    const float ds = w * (dw - attn_wave_sum(w * dw));   // lanes >= N: w = 0, they add nothing and hold ds = 0
    float *dy = dY + r * N * kAttnH;
    float dq = 0.0f;
    for (int t = 0; t < N; ++t) {
        const float wt = attn_lane_value(w, t), dst = attn_lane_value(ds, t);
        dq = fmaf(dst, y[t * kAttnH + j], dq);
        float g = fmaf(dst, q, wt * dc);
        if (t == N - 1) g += dq;   // the last step is also the query
        if (valid) dy[t * kAttnH + j] = g;
    }
}

}  // namespace
