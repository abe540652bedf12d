// libpworld.so, thirteenth translation unit -- the output layers of the learner's networks with gradient (the ReLU on the actor's
// BiLSTM output and every head: dense2 / dense2_1 + dense2_2 / dense3, what actor(s0), critic(s0, a0) and critic(s0, sample(actor(s0)))
// end with): pw_head_train_forward (one launch for all heads), pw_head_train_backward (two: the main kernel and the ordered sum of
// its per-workgroup partial sums; one when a single workgroup holds every row) and pw_head_train_scratch_bytes.  The kernels, their
// mapping and their summation order are csrc/pw_kernels_head.hpp.  Declared in include/pworld.h; the error text is shared with pworld.hip.
#include "pw_host.hpp"
#include "pw_kernels_head.hpp"

namespace {

// what the entry points check of the shape they share
int head_shape(int64_t rows, int32_t heads, const int32_t *n)
{
    if (heads < 1 || heads > kHeadMaxHeads) return fail(PW_EINVAL, "heads must be in [1, 3]");
    if (!n) return fail(PW_EINVAL, "null argument: n");
    for (int k = 0; k < heads; ++k)
        if (n[k] < 1 || n[k] > kHeadMaxN) return fail(PW_EINVAL, "n: every head holds 1 to 104 columns");
    if (const char *why = train_rows_refused(rows)) return fail(PW_EINVAL, why);
    return PW_OK;
}

}  // namespace

extern "C" {

size_t pw_head_train_scratch_bytes(int64_t rows, int32_t heads, const int32_t *n)
{
    if (rows < 1 || heads < 1 || heads > kHeadMaxHeads || !n) return 0;
    size_t per_slot = 0;
    for (int k = 0; k < heads; ++k) {
        if (n[k] < 1 || n[k] > kHeadMaxN) return 0;
        per_slot += (size_t)head_partial_floats(n[k]);
    }
    return train_scratch_bytes((long)rows, per_slot);
}

int pw_head_train_forward(const float *X, int64_t rows, int32_t relu, int32_t heads, const float *const *w, const float *const *b,
                          const int32_t *n, float *const *out, void *stream)
{
    if (int rc = head_shape(rows, heads, n)) return rc;
    if (!X || !w || !b || !out) return fail(PW_EINVAL, "null argument");
    HeadFwdArgs A = {};
    for (int k = 0; k < heads; ++k) {
        if (!w[k] || !b[k] || !out[k]) return fail(PW_EINVAL, "w, b and out: one tensor per head");
        if (misaligned(w[k]) || misaligned(b[k]) || misaligned(out[k])) return fail(PW_EINVAL, "every pointer must be 4-byte aligned");
        A.w[k] = w[k]; A.b[k] = b[k]; A.out[k] = out[k]; A.n[k] = n[k];
    }
    if (misaligned(X)) return fail(PW_EINVAL, "every pointer must be 4-byte aligned");
    A.x = X; A.rows = (long)rows; A.heads = heads; A.relu = relu != 0;
    const long groups = (A.rows + kHeadFwdRows - 1) / kHeadFwdRows;
    hipLaunchKernelGGL(pw_head_train_forward_kernel, dim3((unsigned)groups), dim3(kTrainThreads), head_lds(false).bytes,
                       static_cast<hipStream_t>(stream), A);
    PW_HIP_CHECK(hipGetLastError());
    return PW_OK;
}

int pw_head_train_backward(const float *const *dOut, const float *X, int64_t rows, int32_t relu, int32_t heads, const float *const *w,
                           const int32_t *n, float *dX, float *const *dW, float *const *db, void *scratch, size_t scratch_bytes,
                           void *stream)
{
    if (int rc = head_shape(rows, heads, n)) return rc;
    if (!dOut || !X || !w || !dW || !db || !scratch) return fail(PW_EINVAL, "null argument");
    if (misaligned(X) || misaligned(scratch)) return fail(PW_EINVAL, "every pointer must be 4-byte aligned");
    if (misaligned(dX, 16)) return fail(PW_EINVAL, "dX must be 16-byte aligned");
    if (scratch_bytes < pw_head_train_scratch_bytes(rows, heads, n))
        return fail(PW_EINVAL, "scratch_bytes is less than pw_head_train_scratch_bytes(rows, heads, n)");
    const TrainSplit S = train_split((long)rows);
    HeadBwdArgs A = {};
    HeadReduceArgs R = {};
    int used = 0, tiles = 0, floats = 0;
    for (int k = 0; k < heads; ++k) {
        if (!dOut[k]) {   // the head received no gradient: it is not part of the launch
            if (dW[k] || db[k]) return fail(PW_EINVAL, "dW and db of a head whose dOut is NULL must be NULL");
            continue;
        }
        if (!w[k] || !dW[k] || !db[k]) return fail(PW_EINVAL, "w, dW and db: one tensor per head that has a dOut");
        if (misaligned(dOut[k]) || misaligned(w[k]) || misaligned(dW[k]) || misaligned(db[k]))
            return fail(PW_EINVAL, "every pointer must be 4-byte aligned");
        A.dout[used] = dOut[k]; A.w[used] = w[k]; A.dw[used] = R.dw[used] = dW[k]; A.db[used] = R.db[used] = db[k];
        A.n[used] = R.n[used] = n[k]; A.tile0[used] = tiles; A.base[used] = R.base[used] = floats;
        tiles += (n[k] + kTrainTile - 1) / kTrainTile; floats += (int)head_partial_floats(n[k]);
        ++used;
    }
    if (!used) return fail(PW_EINVAL, "dOut: every head's is NULL, there is nothing to compute");
    A.x = X; A.partial = static_cast<float *>(scratch); A.dx = dX;
    A.rows = (long)rows; A.per_group = S.per_group; A.per_slot = floats;
    A.heads = used; A.relu = relu != 0; A.ntiles = tiles; A.direct = S.groups == 1;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(pw_head_train_backward_kernel, dim3((unsigned)S.groups), dim3(kTrainThreads), head_lds(true).bytes, s, A);
    PW_HIP_CHECK(hipGetLastError());
    if (A.direct) return PW_OK;
    R.partial = A.partial; R.per_slot = floats; R.heads = used; R.groups = S.groups;
    hipLaunchKernelGGL(pw_head_train_reduce_kernel, dim3(train_reduce_blocks(R.per_slot)), dim3(kTrainThreads), 0, s, R);
    PW_HIP_CHECK(hipGetLastError());
    return PW_OK;
}

}  // extern "C"
