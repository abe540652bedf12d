// pw_lstm_math.hpp -- part of libpworld.so: the device functions the actor (pw_kernels_policy.hpp, pw_kernels_actor16.hpp) and
// the critic (pw_kernels_critic.hpp) share -- gate activations, the LSTM cell, the LDS-only workgroup barrier, the lane
// exchanges, the MFMA accumulator type.  No kernel is defined here.
#pragma once

#include <hip/hip_runtime.h>

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// v_exp_f32 / v_rcp_f32 (1 ulp): the policy net is ordinary float32 inference, not part of the
// bit-exact environment contract; tests compare against PyTorch's float32 LSTM with a 2e-5 bound.
__device__ __forceinline__ float fast_sigmoid(float x) { return __builtin_amdgcn_rcpf(1.0f + __expf(-x)); }
// tanh(x) = 2 / (1 + exp(-2x)) - 1: five instructions (mul, exp2, add, rcp, fma) instead of the nine of (1 - e) / (1 + e) on |x| with the
// sign copied back -- the cell update is vector work that cannot overlap the exact-f32 matrix instructions, so every instruction of it
// is on the timestep's path (round 5: 2 % of a step).  x -> -inf: exp = inf, rcp = 0, result -1; x -> +inf: exp = 0, result 1; no NaN from
// finite input.  Same absolute accuracy as the other form (both are limited by the rounding of a number near 1: ~1e-7).
__device__ __forceinline__ float fast_tanh(float x)
{
    return fmaf(2.0f, __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(x * -2.8853900817779268f)), -1.0f);   // exp(-2x) = 2^(-2 log2(e) x): one multiply
}

// The forward ReLU of every network kernel.  NaN -> NaN, as torch.relu and the float64 restatements have it: fmaxf(v, 0) is v_max_f32,
// which returns the other operand for a NaN, i.e. turns a poisoned row into hid = 0 and a finite loss.  IEEE 754-2019's maximum
// carries the NaN and, like v_max_f32, orders -0 below +0, so every other input keeps the bits fmaxf gave it; on gfx950 it is one
// instruction as before (v_maximum3_f32 v, v, 0, 0).  The compare-and-select spelling "!(v <= 0) ? v : 0" computes the same but
// costs an instruction per value and took the simple_tag policy rollout (at the 256-register cap) into spilling.
__device__ __forceinline__ float relu_fwd(const float v) { return __builtin_elementwise_maximum(v, 0.0f); }

// One LSTM cell (PyTorch's gate order i, f, g, o): pre-activations -> new cell state c and output h.  Every kernel form calls this
// one function, so the forms agree bit for bit whatever the activations' rounding is.
// (The four gates' exponent arguments and denominators are formed two at a time -- (i, f) and (g, o) sit in adjacent accumulator registers --
// so that they compile to packed multiplies / adds; the operations and their bits are those of fast_sigmoid / fast_tanh.)
__device__ __forceinline__ void lstm_cell(const float gi, const float gf, const float gg, const float go, float &c, float &h)
{
    typedef float v2 __attribute__((ext_vector_type(2)));
    const v2 a = v2{gi, gf} * v2{-1.4426950408889634f, -1.4426950408889634f};   // exp(-x) = 2^(-log2(e) x)
    const v2 b = v2{gg, go} * v2{-2.8853900817779268f, -1.4426950408889634f};   // tanh's exp(-2x) for g
    const v2 d1 = v2{__builtin_amdgcn_exp2f(a.x), __builtin_amdgcn_exp2f(a.y)} + v2{1.0f, 1.0f};
    const v2 d2 = v2{__builtin_amdgcn_exp2f(b.x), __builtin_amdgcn_exp2f(b.y)} + v2{1.0f, 1.0f};
    const float si = __builtin_amdgcn_rcpf(d1.x), sf = __builtin_amdgcn_rcpf(d1.y), so = __builtin_amdgcn_rcpf(d2.y);
    const float tg = fmaf(2.0f, __builtin_amdgcn_rcpf(d2.x), -1.0f);
    c = sf * c + si * tg;
    h = so * fast_tanh(c);
}

// Workgroup barrier that orders LDS traffic only.  __syncthreads() also carries a workgroup-scope fence for GLOBAL
// memory, i.e. an s_waitcnt vmcnt(0): every wave would sit out the full HBM latency of its outstanding stores at
// each of the ~8 barriers of a pass.  Inside these kernels waves hand data to each other through LDS alone, and
// what they store to global memory is only read after the kernel (or behind an explicit __threadfence).
__device__ __forceinline__ void wg_lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// The value of lane ^ 16 / lane ^ 32 by v_permlane16_swap / v_permlane32_swap (gfx950): the instruction swaps the odd rows (halves) of
// its first operand with the even rows (halves) of the second, so with both operands the same value the first holds, in every
// even row (half), its own value and the second its neighbour's -- one VALU instruction and a select instead of a ds_bpermute
// round trip through the LDS crossbar (~120 cycles, exposed on the head's dependent chain).
__device__ __forceinline__ uint32_t lane_xor16(const uint32_t v)
{
    const auto r = __builtin_amdgcn_permlane16_swap(v, v, false, false);
    return (threadIdx.x & 16) ? r[0] : r[1];
}
__device__ __forceinline__ uint32_t lane_xor32(const uint32_t v)
{
    const auto r = __builtin_amdgcn_permlane32_swap(v, v, false, false);
    return (threadIdx.x & 32) ? r[0] : r[1];
}
__device__ __forceinline__ float lane_xor16(const float v) { return __uint_as_float(lane_xor16(__float_as_uint(v))); }
__device__ __forceinline__ float lane_xor32(const float v) { return __uint_as_float(lane_xor32(__float_as_uint(v))); }

}  // namespace
