// libpworld.so, tenth translation unit -- the learner's straight-through Gumbel-softmax sample with gradient (the sampling of a1 from the
// target actor's logits and of the actor loss's action; ddpg_gumbel_fix.py:150, :178): pw_gumbel_st_forward and pw_gumbel_st_backward, one
// launch each.  The kernels, their mapping, the noise's key and the summation order are csrc/pw_kernels_sample.hpp.  Declared in
// include/pworld.h; the error text is shared with pworld.hip.
#include "pw_host.hpp"
#include "pw_kernels_sample.hpp"

namespace {

// what both entry points check of their shared arguments
int sample_args(int64_t rows, int32_t n, float tau)
{
    if (n < 1 || n > kSampleMaxLogits) return fail(PW_EINVAL, "n must be in 1 .. 16");
    if (!(tau > 0.0f) || !(tau <= 3.0e38f)) return fail(PW_EINVAL, "tau must be a finite number > 0");
    if (rows < 1) return fail(PW_EINVAL, "rows must be >= 1");
    if (rows > (int64_t)0x7fffffff * kSampleThreads) return fail(PW_EINVAL, "rows: more rows than one launch's grid holds");
    return PW_OK;
}

unsigned sample_grid(int64_t rows) { return (unsigned)((rows + kSampleThreads - 1) / kSampleThreads); }

}  // namespace

extern "C" {

int pw_gumbel_st_forward(const float *logits, int64_t rows, int32_t n, float tau, int32_t hard, uint64_t seed, uint64_t step,
                         const int64_t *step_dev, float *y, float *soft, int32_t *idx, float *noise, void *stream)
{
    if (int rc = sample_args(rows, n, tau)) return rc;
    if (!logits) return fail(PW_EINVAL, "logits is null");
    if (!y) return fail(PW_EINVAL, "y is null");
    if (misaligned(logits)) return fail(PW_EINVAL, "logits must be 4-byte aligned");
    if (misaligned(y)) return fail(PW_EINVAL, "y must be 4-byte aligned");
    if (misaligned(soft)) return fail(PW_EINVAL, "soft must be 4-byte aligned");
    if (misaligned(idx)) return fail(PW_EINVAL, "idx must be 4-byte aligned");
    if (misaligned(noise)) return fail(PW_EINVAL, "noise must be 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(step_dev) & 7u) return fail(PW_EINVAL, "step_dev must be 8-byte aligned");
    const dim3 grid(sample_grid(rows)), block(kSampleThreads);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int h = hard ? 1 : 0;
#define PW_SAMPLE_FWD(NB)                                                                                                          \
    hipLaunchKernelGGL(pw_gumbel_st_forward_kernel<NB>, grid, block, 0, s, logits, (long)rows, n, tau, h, seed, step, step_dev, y, \
                       soft, idx, noise)
    switch ((n + 3) / 4) {
        case 1: PW_SAMPLE_FWD(1); break;
        case 2: PW_SAMPLE_FWD(2); break;
        case 3: PW_SAMPLE_FWD(3); break;
        default: PW_SAMPLE_FWD(4); break;
    }
#undef PW_SAMPLE_FWD
    PW_HIP_CHECK(hipGetLastError());
    return PW_OK;
}

int pw_gumbel_st_backward(const float *dY, const float *soft, int64_t rows, int32_t n, float tau, float *dLogits, void *stream)
{
    if (int rc = sample_args(rows, n, tau)) return rc;
    if (!dY) return fail(PW_EINVAL, "dY is null");
    if (!soft) return fail(PW_EINVAL, "soft is null");
    if (!dLogits) return fail(PW_EINVAL, "dLogits is null");
    if (misaligned(dY)) return fail(PW_EINVAL, "dY must be 4-byte aligned");
    if (misaligned(soft)) return fail(PW_EINVAL, "soft must be 4-byte aligned");
    if (misaligned(dLogits)) return fail(PW_EINVAL, "dLogits must be 4-byte aligned");
    const dim3 grid(sample_grid(rows)), block(kSampleThreads);
    hipStream_t s = static_cast<hipStream_t>(stream);
#define PW_SAMPLE_BWD(NB) \
    hipLaunchKernelGGL(pw_gumbel_st_backward_kernel<NB>, grid, block, 0, s, dY, soft, (long)rows, n, tau, dLogits)
    switch ((n + 3) / 4) {
        case 1: PW_SAMPLE_BWD(1); break;
        case 2: PW_SAMPLE_BWD(2); break;
        case 3: PW_SAMPLE_BWD(3); break;
        default: PW_SAMPLE_BWD(4); break;
    }
#undef PW_SAMPLE_BWD
    PW_HIP_CHECK(hipGetLastError());
    return PW_OK;
}

}  // extern "C"
