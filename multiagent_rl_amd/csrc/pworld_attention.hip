// libpworld.so, eighth translation unit -- the attention block of the learner's critic with gradient (critic(s0, a0) and
// critic(s0, actor(s0)); critic.py CriticNetwork.forward): pw_attention_pool_forward and pw_attention_pool_backward, one launch each.
// The kernels, their mapping and their summation order are csrc/pw_kernels_attention.hpp.  Declared in include/pworld.h; the error
// text is shared with pworld.hip.
#include "pw_host.hpp"
#include "pw_kernels_attention.hpp"

namespace {

// what both entry points check of their shared arguments
int attention_args(const float *Y, int64_t b, int32_t N, int32_t H)
{
    if (H != kAttnH) return fail(PW_EINVAL, "H: the hidden size served is H = 64");
    if (N < 1 || N > kAttnMaxSteps) return fail(PW_EINVAL, "N must be in 1 .. 64");
    if (b < 1) return fail(PW_EINVAL, "b must be >= 1");
    if (b > (int64_t)0x7fffffff * (kAttnThreads / kAttnH)) return fail(PW_EINVAL, "b: more rows than one launch's grid holds");
    if (!Y) return fail(PW_EINVAL, "Y is null");
    if (misaligned(Y)) return fail(PW_EINVAL, "Y must be 4-byte aligned");
    return PW_OK;
}

unsigned attention_grid(int64_t b)
{
    constexpr int per_group = kAttnThreads / kAttnH;
    return (unsigned)((b + per_group - 1) / per_group);
}

}  // namespace

extern "C" {

int pw_attention_pool_forward(const float *Y, int64_t b, int32_t N, int32_t H, int32_t relu, float *out, float *weight, void *stream)
{
    if (int rc = attention_args(Y, b, N, H)) return rc;
    if (!out) return fail(PW_EINVAL, "out is null");
    if (misaligned(out)) return fail(PW_EINVAL, "out must be 4-byte aligned");
    if (misaligned(weight)) return fail(PW_EINVAL, "weight must be 4-byte aligned");
    hipLaunchKernelGGL(pw_attention_pool_forward_kernel, dim3(attention_grid(b)), dim3(kAttnThreads), 0, static_cast<hipStream_t>(stream),
                       Y, (long)b, N, relu, out, weight);
    PW_HIP_CHECK(hipGetLastError());
    return PW_OK;
}

int pw_attention_pool_backward(const float *dOut, const float *Y, const float *weight, const float *out, int64_t b, int32_t N, int32_t H,
                               int32_t relu, float *dY, void *stream)
{
    if (int rc = attention_args(Y, b, N, H)) return rc;
    if (!dOut) return fail(PW_EINVAL, "dOut is null");
    if (!weight) return fail(PW_EINVAL, "weight is null");
    if (!out) return fail(PW_EINVAL, "out is null");
    if (!dY) return fail(PW_EINVAL, "dY is null");
    if (misaligned(dOut)) return fail(PW_EINVAL, "dOut must be 4-byte aligned");
    if (misaligned(weight)) return fail(PW_EINVAL, "weight must be 4-byte aligned");
    if (misaligned(out)) return fail(PW_EINVAL, "out must be 4-byte aligned");
    if (misaligned(dY)) return fail(PW_EINVAL, "dY must be 4-byte aligned");
    hipLaunchKernelGGL(pw_attention_pool_backward_kernel, dim3(attention_grid(b)), dim3(kAttnThreads), 0, static_cast<hipStream_t>(stream),
                       dOut, Y, weight, out, (long)b, N, relu, dY);
    PW_HIP_CHECK(hipGetLastError());
    return PW_OK;
}

}  // extern "C"
