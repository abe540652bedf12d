// pw_optim_args.hpp -- the argument blocks and the small device functions of the optimiser kernels (no kernel here): shared by
// pw_kernels_optim.hpp (pw_adam_step_kernel, pw_soft_update_kernel; unit csrc/pworld_optim.hip) and pw_kernels_optim_dev.hpp
// (pw_adam_step_dev_kernel; unit csrc/pworld_optim_dev.hip), so that neither unit compiles the other's kernels.
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

}  // namespace
