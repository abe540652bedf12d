// pw_optim_host.hpp -- the host side the optimiser entry points share (csrc/pworld_optim.hip: pw_adam_step, pw_soft_update;
// csrc/pworld_optim_dev.hip: pw_adam_step_dev): argument checks, the tensor table, the tile list.
#pragma once

#include <cmath>

#include "pw_host.hpp"
#include "pw_optim_args.hpp"

namespace {

constexpr int64_t kOptMaxElements = (int64_t)1 << 20;

// tile_begin[] of a table whose tensor k has numel(k) elements; refuses what the launch form does not serve.
template <typename Args, typename Numel>
int opt_tiles(Args &A, int32_t count, Numel numel)
{
    int64_t total = 0;
    A.tile_begin[0] = 0;
    for (int k = 0; k < count; ++k) {
        const int64_t n = numel(k);
        if (n < 1) return fail(PW_EINVAL, "every tensor needs numel >= 1");
        total += n;
        if (total > kOptMaxElements) return fail(PW_EINVAL, "more than 2^20 elements in one call");
        A.tile_begin[k + 1] = A.tile_begin[k] + (int)((n + kOptTile - 1) / kOptTile);
    }
    for (int k = count; k < PW_OPT_MAX_TENSORS; ++k) A.tile_begin[k + 1] = A.tile_begin[count];
    A.count = count;
    return PW_OK;
}

// tau as both kernels use it: (float)tau, (float)(1 - tau) with the difference formed in float64, and the tau == 1 copy
template <typename Args>
void opt_tau(Args &A, double tau)
{
    A.tau = (float)tau;
    A.omt = (float)(1.0 - tau);
    A.hard = tau == 1.0;
}

// Everything of a pw_adam_step / pw_adam_step_dev call but the two step-dependent scalars: checks, the table, the tiles.
int adam_args(OptArgs &A, const pw_opt_tensor *tensors, int32_t count, double lr, double beta1, double beta2, double eps,
              double weight_decay, double max_norm, double tau, float *total_norm)
{
    if (count < 1 || count > PW_OPT_MAX_TENSORS) return fail(PW_EINVAL, "count must be in [1, 32]");
    if (!(lr >= 0.0) || !std::isfinite(lr)) return fail(PW_EINVAL, "lr must be finite and >= 0");
    if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0)) return fail(PW_EINVAL, "beta1, beta2 must be in [0, 1)");
    if (!(eps >= 0.0) || !std::isfinite(eps)) return fail(PW_EINVAL, "eps must be finite and >= 0");
    if (!(weight_decay >= 0.0) || !std::isfinite(weight_decay)) return fail(PW_EINVAL, "weight_decay must be finite and >= 0");
    if (std::isnan(max_norm)) return fail(PW_EINVAL, "max_norm is NaN");
    if (misaligned(total_norm)) return fail(PW_EINVAL, "total_norm must be 4-byte aligned");
    bool any_target = false;
    for (int k = 0; k < count; ++k) {
        const pw_opt_tensor &t = tensors[k];
        if (!t.param || !t.grad || !t.exp_avg || !t.exp_avg_sq) return fail(PW_EINVAL, "null param / grad / exp_avg / exp_avg_sq");
        if (misaligned(t.param) || misaligned(t.grad) || misaligned(t.exp_avg) || misaligned(t.exp_avg_sq) || misaligned(t.target))
            return fail(PW_EINVAL, "tensors must be 4-byte aligned");
        any_target = any_target || t.target != nullptr;
        A.t[k] = OptTensor{t.param, t.grad, t.exp_avg, t.exp_avg_sq, t.target, (long)t.numel};
    }
    for (int k = count; k < PW_OPT_MAX_TENSORS; ++k) A.t[k] = OptTensor{nullptr, nullptr, nullptr, nullptr, nullptr, 0};
    if (any_target && !(tau >= 0.0 && tau <= 1.0)) return fail(PW_EINVAL, "tau must be in [0, 1]");
    if (const int rc = opt_tiles(A, count, [&](int k) { return tensors[k].numel; })) return rc;
    A.need_norm = (max_norm > 0.0 || total_norm != nullptr) ? 1 : 0;
    A.max_norm = max_norm;
    A.wd = (float)weight_decay;
    A.beta1 = (float)beta1; A.beta2 = (float)beta2;
    A.omb1 = (float)(1.0 - beta1); A.omb2 = (float)(1.0 - beta2);
    A.eps = (float)eps;
    A.bc2_sqrt = 1.0f; A.step_size = 0.0f;   // the caller's
    opt_tau(A, any_target ? tau : 0.0);
    A.total_norm = total_norm;
    return PW_OK;
}

}  // namespace
