// libpworld.so, seventh translation unit -- the recurrent part of a one-layer LSTM with gradient for the learner's passes
// (critic(s0, a0), actor(s0), critic(s0, actor(s0)); ddpg_gumbel_fix.py:156-206): pw_lstm_train_forward and
// pw_lstm_train_backward, one launch each.  The kernels, their mapping and their summation order are csrc/pw_kernels_lstm.hpp; the
// gate functions are the actor's (pw_lstm_math.hpp: included, not copied).  Declared in include/pworld.h; the error text is
// shared with pworld.hip.
#include "pw_host.hpp"
#include "pw_kernels_lstm.hpp"

namespace {

// what both entry points check of their shared arguments; *groups = b * dirs (one per sequence and direction)
int lstm_args(const float *w_hh_fw, const float *w_hh_bw, int64_t b, int32_t N, int32_t dirs, int32_t H, int64_t *groups)
{
    if (!((dirs == 1 && H == 64) || (dirs == 2 && H == 32)))
        return fail(PW_EINVAL, "dirs / H: the shapes served are dirs = 1, H = 64 and dirs = 2, H = 32");
    if (N < 1) return fail(PW_EINVAL, "N must be >= 1");
    if (b < 1) return fail(PW_EINVAL, "b must be >= 1");
    if (!w_hh_fw) return fail(PW_EINVAL, "w_hh_fw is null");
    if (dirs == 2 && !w_hh_bw) return fail(PW_EINVAL, "w_hh_bw is null with dirs = 2");
    if (dirs == 1 && w_hh_bw) return fail(PW_EINVAL, "w_hh_bw must be null with dirs = 1");
    if (misaligned(w_hh_fw)) return fail(PW_EINVAL, "w_hh_fw must be 4-byte aligned");
    if (misaligned(w_hh_bw)) return fail(PW_EINVAL, "w_hh_bw must be 4-byte aligned");
    const int64_t per_group = kLstmThreads / H;
    if (b > ((int64_t)0x7fffffff * per_group) / dirs) return fail(PW_EINVAL, "b: more sequences than one launch's grid holds");
    *groups = b * dirs;
    return PW_OK;
}

template <int H, int DIRS>
int lstm_forward_launch(const float *G, const float *w_fw, const float *w_bw, int64_t b, int32_t N, int64_t groups, float *Y,
                        float *saved, hipStream_t stream)
{
    static unsigned long long optin_mask = 0;
    const auto kernel = pw_lstm_train_forward_kernel<H, DIRS>;
    const size_t lds = lstm_train_lds(H, DIRS, false).bytes;
    PW_LDS_OPTIN(&optin_mask, kernel);
    constexpr int per_group = kLstmThreads / H;
    hipLaunchKernelGGL(kernel, dim3((unsigned)((groups + per_group - 1) / per_group)), dim3(kLstmThreads), lds, stream, G, w_fw, w_bw,
                       (long)b, N, Y, saved);
    PW_HIP_CHECK(hipGetLastError());
    return PW_OK;
}

template <int H, int DIRS>
int lstm_backward_launch(const float *dY, const float *saved, const float *w_fw, const float *w_bw, int64_t b, int32_t N,
                         int64_t groups, float *dG, hipStream_t stream)
{
    static unsigned long long optin_mask = 0;
    const auto kernel = pw_lstm_train_backward_kernel<H, DIRS>;
    const size_t lds = lstm_train_lds(H, DIRS, true).bytes;
    PW_LDS_OPTIN(&optin_mask, kernel);
    constexpr int per_group = kLstmThreads / H;
    hipLaunchKernelGGL(kernel, dim3((unsigned)((groups + per_group - 1) / per_group)), dim3(kLstmThreads), lds, stream, dY, saved,
                       w_fw, w_bw, (long)b, N, dG);
    PW_HIP_CHECK(hipGetLastError());
    return PW_OK;
}

}  // namespace

extern "C" {

int pw_lstm_train_forward(const float *G, const float *w_hh_fw, const float *w_hh_bw, int64_t b, int32_t N, int32_t dirs, int32_t H,
                          float *Y, float *saved, void *stream)
{
    int64_t groups = 0;
    if (int rc = lstm_args(w_hh_fw, w_hh_bw, b, N, dirs, H, &groups)) return rc;
    if (!G) return fail(PW_EINVAL, "G is null");
    if (!Y) return fail(PW_EINVAL, "Y is null");
    if (misaligned(G)) return fail(PW_EINVAL, "G must be 4-byte aligned");
    if (misaligned(Y)) return fail(PW_EINVAL, "Y must be 4-byte aligned");
    if (misaligned(saved)) return fail(PW_EINVAL, "saved must be 4-byte aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    return dirs == 1 ? lstm_forward_launch<64, 1>(G, w_hh_fw, w_hh_bw, b, N, groups, Y, saved, s)
                     : lstm_forward_launch<32, 2>(G, w_hh_fw, w_hh_bw, b, N, groups, Y, saved, s);
}

int pw_lstm_train_backward(const float *dY, const float *saved, const float *w_hh_fw, const float *w_hh_bw, int64_t b, int32_t N,
                           int32_t dirs, int32_t H, float *dG, void *stream)
{
    int64_t groups = 0;
    if (int rc = lstm_args(w_hh_fw, w_hh_bw, b, N, dirs, H, &groups)) return rc;
    if (!dY) return fail(PW_EINVAL, "dY is null");
    if (!saved) return fail(PW_EINVAL, "saved is null");
    if (!dG) return fail(PW_EINVAL, "dG is null");
    if (misaligned(dY)) return fail(PW_EINVAL, "dY must be 4-byte aligned");
    if (misaligned(saved)) return fail(PW_EINVAL, "saved must be 4-byte aligned");
    if (misaligned(dG)) return fail(PW_EINVAL, "dG must be 4-byte aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    return dirs == 1 ? lstm_backward_launch<64, 1>(dY, saved, w_hh_fw, w_hh_bw, b, N, groups, dG, s)
                     : lstm_backward_launch<32, 2>(dY, saved, w_hh_fw, w_hh_bw, b, N, groups, dG, s);
}

}  // extern "C"
