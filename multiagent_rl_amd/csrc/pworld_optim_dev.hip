// libpworld.so, ninth translation unit -- pw_adam_step_dev: pw_adam_step (csrc/pworld_optim.hip) with the step count read from device
// memory and the bias corrections formed in the kernel, for an update that is captured once and replayed (multiagent_rl_amd/graph.py),
// and pw_adam_bias_scalars, the same scalars on the host.  A unit of its own: csrc/pworld_optim.hip carries exactly the kernels of
// pw_kernels_optim.hpp.  Declared in include/pworld.h; the error text is shared with pworld.hip.
#include "pw_optim_host.hpp"
#include "pw_kernels_optim_dev.hpp"

extern "C" {

void pw_adam_bias_scalars(int64_t step, double lr, double beta1, double beta2, float out[2])
{
    pw_adam_bias(step, lr, beta1, beta2, &out[0], &out[1]);
}

int pw_adam_step_dev(const pw_opt_tensor *tensors, int32_t count, const int64_t *step_dev, double lr, double beta1, double beta2,
                     double eps, double weight_decay, double max_norm, double tau, float *total_norm, void *stream)
{
    if (!tensors) return fail(PW_EINVAL, "pw_adam_step_dev: tensors is null");
    if (!step_dev) return fail(PW_EINVAL, "pw_adam_step_dev: step_dev is null (the device cell that holds the step this call takes)");
    if (reinterpret_cast<uintptr_t>(step_dev) & 7) return fail(PW_EINVAL, "pw_adam_step_dev: step_dev must be 8-byte aligned");
    OptArgs A;
    if (const int rc = adam_args(A, tensors, count, lr, beta1, beta2, eps, weight_decay, max_norm, tau, total_norm)) return rc;
    hipLaunchKernelGGL(pw_adam_step_dev_kernel, dim3((unsigned)A.tile_begin[count]), dim3(kOptThreads), 0,
                       static_cast<hipStream_t>(stream), A, step_dev, lr, beta1, beta2);
    PW_HIP_CHECK(hipGetLastError());
    return PW_OK;
}

}  // extern "C"
