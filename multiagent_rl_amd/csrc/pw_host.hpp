// pw_host.hpp -- part of libpworld.so: the host plumbing every translation unit uses (error text, HIP error check, the
// LDS opt-in, and the small argument checks the ring and wire entry points share).  No device code, no kernel types.
#pragma once

#include <hip/hip_runtime.h>

#include <string>

#include "pworld.h"

// libpworld.so is eight translation units (pworld.hip: environment; pworld_replay.hip: replay ring, wire blocks; pworld_policy.hip: actor,
// policy rollouts; pworld_policy_generic.hip: the generic policy rollout; pworld_critic.hip; pworld_optim.hip; pworld_lstm.hip; pworld_attention.hip).  The thread-local error text lives in pworld.hip; all reach it through this hook.
extern "C" __attribute__((visibility("hidden"))) void pw_internal_set_error(const char *msg);
// pworld_policy_generic.hip: the launcher of pw_policy_rollout_generic_kernel; pw_policy_rollout (pworld_policy.hip) has checked the
// handle, the weights, io and num_steps and hands everything else over.
extern "C" __attribute__((visibility("hidden"))) int pw_internal_policy_rollout_generic(
    pw_handle *h, const float *frag, const float *b1, const float *b_ih, const float *w_hh_fw, const float *w_hh_bw, const float *w2,
    const float *b2, int32_t relu_out, uint64_t seed, uint64_t step, const int64_t *step_dev, const pw_step_io *io, int32_t *act_out,
    int32_t num_steps, const pw_rollout_sink *sink, void *stream);

namespace {

int fail(int code, const std::string &msg)
{
    pw_internal_set_error(msg.c_str());
    return code;
}

#define PW_HIP_CHECK(expr)                                                             \
    do {                                                                               \
        hipError_t _e = (expr);                                                        \
        if (_e != hipSuccess)                                                          \
            return fail(PW_EHIP, std::string(#expr) + ": " + hipGetErrorString(_e));   \
    } while (0)

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// the address is no multiple of `to` (a power of two); NULL is aligned
bool misaligned(const void *p, uintptr_t to = 4) { return (reinterpret_cast<uintptr_t>(p) & (to - 1)) != 0; }

// Kernels that ask for more than 64 KB of dynamic LDS need the opt-in once per (kernel, DEVICE): a process driving
// several GPUs must not skip it on the second one.  The device's bit is set only AFTER hipFuncSetAttribute succeeded
// (lds_optin_done), atomically: a failed call is retried by the next launch, and two host threads on different devices
// cannot lose each other's bit.
bool lds_optin_needed(const unsigned long long *done_mask, int *dev_out)
{
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) { *dev_out = -1; return true; }  // unknown: set it every time (cheap)
    *dev_out = dev;
    return !(__atomic_load_n(done_mask, __ATOMIC_ACQUIRE) >> dev & 1ull);
}

void lds_optin_done(unsigned long long *done_mask, int dev)
{
    if (dev >= 0) __atomic_fetch_or(done_mask, 1ull << dev, __ATOMIC_RELEASE);
}

// hipFuncSetAttribute(kernel, MaxDynamicSharedMemorySize, 160 KB) once per (kernel, device); returns from the caller on failure
#define PW_LDS_OPTIN(mask_ptr, kernel_expr)                                                                              \
    do {                                                                                                                 \
        int optin_dev_;                                                                                                  \
        if (lds_optin_needed((mask_ptr), &optin_dev_)) {                                                                 \
            PW_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel_expr),                                \
                                             hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));                   \
            lds_optin_done((mask_ptr), optin_dev_);                                                                      \
        }                                                                                                                \
    } while (0)

// Workgroups of 256 threads that cover `total` items, at most `cap` of them (the kernels stride over the rest).
unsigned grid_blocks(size_t total, size_t cap) { return (unsigned)((total + 255) / 256 > cap ? cap : (total + 255) / 256); }

// F = the most episode ends one env can see in a chunk of T steps (0 without an episode limit); each wire format has its `limit`.
int episode_ends_per_chunk(int32_t T, int32_t max_episode_len, int limit, int32_t *F)
{
    const int64_t f = max_episode_len > 0 ? ((int64_t)T + max_episode_len - 1) / max_episode_len : 0;
    if (f > limit)
        return fail(PW_EINVAL, "more than " + std::to_string(limit) + " episode ends per env and chunk: use shorter chunks");
    *F = (int32_t)f;
    return PW_OK;
}

// `rows` new transitions fit the ring and the cursor is a valid one (the caller has checked rows >= 1).
bool ring_fits(const pw_replay_store *st, int64_t rows, int64_t start) { return st->capacity >= 1 && rows <= st->capacity && start >= 0; }

// Lays the planes of a wire block out one behind the other, each on a 256-byte boundary.
struct PlaneAllocator {
    size_t off = 0;
    size_t operator()(size_t bytes) { const size_t o = off; off = align_up(off + bytes, 256); return o; }
};

}  // namespace
