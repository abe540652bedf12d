// libpworld.so, fourth translation unit -- the tail of the learner's update: pw_adam_step (global-norm clip + Adam + Polyak
// update of the target network, ddpg_gumbel_fix.py:172-173,208-213) and pw_soft_update (:36-47), one launch each.  The kernels
// and their arithmetic order are csrc/pw_kernels_optim.hpp.  Declared in include/pworld.h; the error text is shared with
// pworld.hip.
#include "pw_optim_host.hpp"
#include "pw_kernels_optim.hpp"

extern "C" {

int pw_adam_step(const pw_opt_tensor *tensors, int32_t count, int64_t step, double lr, double beta1, double beta2, double eps,
                 double weight_decay, double max_norm, double tau, float *total_norm, void *stream)
{
    if (!tensors) return fail(PW_EINVAL, "null argument");
    if (count < 1 || count > PW_OPT_MAX_TENSORS) return fail(PW_EINVAL, "count must be in [1, 32]");
    if (step < 1) return fail(PW_EINVAL, "step must be >= 1 (the step this call takes)");
    OptArgs A;
    if (const int rc = adam_args(A, tensors, count, lr, beta1, beta2, eps, weight_decay, max_norm, tau, total_norm)) return rc;
    // torch.optim.adam._single_tensor_adam: the bias corrections in float64 from the step count
    const double bc1 = 1.0 - std::pow(beta1, (double)step), bc2 = 1.0 - std::pow(beta2, (double)step);
    A.bc2_sqrt = (float)std::sqrt(bc2);
    A.step_size = (float)(lr / bc1);
    hipLaunchKernelGGL(pw_adam_step_kernel, dim3((unsigned)A.tile_begin[count]), dim3(kOptThreads), 0,
                       static_cast<hipStream_t>(stream), A);
    PW_HIP_CHECK(hipGetLastError());
    return PW_OK;
}

int pw_soft_update(float *const *target, const float *const *source, const int64_t *numel, int32_t count, double tau, void *stream)
{
    if (!target || !source || !numel) return fail(PW_EINVAL, "null argument");
    if (count < 1 || count > PW_OPT_MAX_TENSORS) return fail(PW_EINVAL, "count must be in [1, 32]");
    if (!(tau >= 0.0 && tau <= 1.0)) return fail(PW_EINVAL, "tau must be in [0, 1]");
    SoftArgs A;
    for (int k = 0; k < count; ++k) {
        if (!target[k] || !source[k]) return fail(PW_EINVAL, "null target / source");
        if (misaligned(target[k]) || misaligned(source[k])) return fail(PW_EINVAL, "tensors must be 4-byte aligned");
        A.t[k] = SoftTensor{target[k], source[k], (long)numel[k]};
    }
    for (int k = count; k < PW_OPT_MAX_TENSORS; ++k) A.t[k] = SoftTensor{nullptr, nullptr, 0};
    if (const int rc = opt_tiles(A, count, [&](int k) { return numel[k]; })) return rc;
    opt_tau(A, tau);
    hipLaunchKernelGGL(pw_soft_update_kernel, dim3((unsigned)A.tile_begin[count]), dim3(kOptThreads), 0,
                       static_cast<hipStream_t>(stream), A);
    PW_HIP_CHECK(hipGetLastError());
    return PW_OK;
}

}  // extern "C"
