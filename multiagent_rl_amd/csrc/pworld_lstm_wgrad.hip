// libpworld.so, twelfth translation unit -- dW_hh of the learner's LSTMs: pw_lstm_train_wgrad and pw_lstm_train_wgrad_scratch_bytes,
// the two recurrent-weight gradients (dG^T against the output shifted by one step) of both directions as two launches.  The kernels,
// their mapping and their summation order are csrc/pw_kernels_lstm_wgrad.hpp.  A unit of its own beside pworld_lstm.hip, whose object
// holds the recurrence kernels and nothing else.  Declared in include/pworld.h; the error text is shared with pworld.hip.
#include "pw_host.hpp"
#include "pw_kernels_lstm_wgrad.hpp"

namespace {

template <int H, int DIRS>
int lstm_wgrad_launch(const float *dG, const float *Y, int64_t b, int32_t N, float *dw_fw, float *dw_bw, float *partial, hipStream_t stream)
{
    static unsigned long long optin_mask = 0;
    const auto kernel = pw_lstm_train_wgrad_kernel<H, DIRS>;
    const size_t lds = lstm_wgrad_lds().bytes;
    PW_LDS_OPTIN(&optin_mask, kernel);
    const long rows = (long)b * N;
    const TrainSplit S = train_split(rows);
    const int want = (dw_fw ? 1 : 0) | (dw_bw ? 2 : 0);
    hipLaunchKernelGGL(kernel, dim3((unsigned)S.groups), dim3(kTrainThreads), lds, stream, dG, Y, rows, N, S.per_group, want, partial);
    PW_HIP_CHECK(hipGetLastError());
    const long per_slot = lstm_wgrad_slot_floats(DIRS), per_dir = 4L * H * H;
    hipLaunchKernelGGL(pw_lstm_train_wgrad_reduce_kernel, dim3(train_reduce_blocks(per_slot)), dim3(kTrainThreads), 0, stream, partial,
                       S.groups, per_slot, per_dir, dw_fw, dw_bw);
    PW_HIP_CHECK(hipGetLastError());
    return PW_OK;
}

// what pw_lstm_train_wgrad and its scratch size check of the shape; 0 when it is served
const char *wgrad_shape(int64_t b, int32_t N, int32_t dirs, int32_t H)
{
    if (!((dirs == 1 && H == 64) || (dirs == 2 && H == 32))) return "dirs / H: the shapes served are dirs = 1, H = 64 and dirs = 2, H = 32";
    if (N < 1) return "N must be >= 1";
    if (b < 1) return "b must be >= 1";
    if (b > ((int64_t)1 << 40) / N) return "b N: more rows than one launch serves (2^40)";
    return nullptr;
}

}  // namespace

extern "C" {

size_t pw_lstm_train_wgrad_scratch_bytes(int64_t b, int32_t N, int32_t dirs, int32_t H)
{
    if (wgrad_shape(b, N, dirs, H)) return 0;
    return train_scratch_bytes((long)b * N, (size_t)lstm_wgrad_slot_floats(dirs));
}

int pw_lstm_train_wgrad(const float *dG, const float *Y, int64_t b, int32_t N, int32_t dirs, int32_t H, float *dw_hh_fw, float *dw_hh_bw,
                        void *scratch, void *stream)
{
    if (const char *why = wgrad_shape(b, N, dirs, H)) return fail(PW_EINVAL, why);
    if (!dG) return fail(PW_EINVAL, "dG is null");
    if (!Y) return fail(PW_EINVAL, "Y is null");
    if (!dw_hh_fw && !dw_hh_bw) return fail(PW_EINVAL, "dw_hh_fw and dw_hh_bw are both null: nothing to compute");
    if (dirs == 1 && dw_hh_bw) return fail(PW_EINVAL, "dw_hh_bw must be null with dirs = 1");
    if (!scratch) return fail(PW_EINVAL, "scratch is null (pw_lstm_train_wgrad_scratch_bytes)");
    if (misaligned(dG)) return fail(PW_EINVAL, "dG must be 4-byte aligned");
    if (misaligned(Y)) return fail(PW_EINVAL, "Y must be 4-byte aligned");
    if (misaligned(dw_hh_fw)) return fail(PW_EINVAL, "dw_hh_fw must be 4-byte aligned");
    if (misaligned(dw_hh_bw)) return fail(PW_EINVAL, "dw_hh_bw must be 4-byte aligned");
    if (misaligned(scratch)) return fail(PW_EINVAL, "scratch must be 4-byte aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    float *partial = static_cast<float *>(scratch);
    return dirs == 1 ? lstm_wgrad_launch<64, 1>(dG, Y, b, N, dw_hh_fw, dw_hh_bw, partial, s)
                     : lstm_wgrad_launch<32, 2>(dG, Y, b, N, dw_hh_fw, dw_hh_bw, partial, s);
}

}  // extern "C"
