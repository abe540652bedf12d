// libpworld.so, eleventh translation unit -- the dense front of the learner's networks with gradient (dense1, ReLU and the LSTM's
// input projection, what critic(s0, a0), actor(s0) and critic(s0, sample(actor(s0))) begin with): pw_front_train_forward (one launch),
// pw_front_train_backward (two: the main kernel and the ordered sum of its per-workgroup partial sums) and
// pw_front_train_scratch_bytes.  The kernels, their mapping and their summation order are csrc/pw_kernels_front.hpp.  Declared in
// include/pworld.h; the error text is shared with pworld.hip.
#include "pw_host.hpp"
#include "pw_kernels_front.hpp"

namespace {

// what the entry points check of the shape they share
int front_shape(int64_t rows, int32_t d0, int32_t d1, int32_t dirs, int32_t H)
{
    if (!((dirs == 1 && H == 64) || (dirs == 2 && H == 32)))
        return fail(PW_EINVAL, "(dirs, H): the shapes served are (1, 64) and (2, 32)");
    if (d0 < 1 || d0 > kFrontMaxD0) return fail(PW_EINVAL, "d0 must be in [1, 104]");
    if (d1 < 0 || d1 > kFrontMaxD1) return fail(PW_EINVAL, "d1 must be in [0, 16]");
    if (const char *why = train_rows_refused(rows)) return fail(PW_EINVAL, why);
    return PW_OK;
}

}  // namespace

extern "C" {

size_t pw_front_train_scratch_bytes(int64_t rows, int32_t d0, int32_t d1)
{
    if (rows < 1 || d0 < 1 || d0 > kFrontMaxD0 || d1 < 0 || d1 > kFrontMaxD1) return 0;
    return train_scratch_bytes((long)rows, (size_t)front_partial_floats(d0 + d1));
}

int pw_front_train_forward(const float *x0, int32_t d0, const float *x1, int32_t d1, const float *w1, const float *b1,
                           const float *const w_ih[2], const float *const b_ih[2], const float *const b_hh[2], int64_t rows,
                           int32_t dirs, int32_t H, float *hid, float *G, void *stream)
{
    if (int rc = front_shape(rows, d0, d1, dirs, H)) return rc;
    if (!x0 || !w1 || !b1 || !w_ih || !b_ih || !b_hh || !G) return fail(PW_EINVAL, "null argument");
    if ((x1 != nullptr) != (d1 > 0)) return fail(PW_EINVAL, "x1 comes with d1 > 0 and only then");
    FrontFwdArgs A;
    A.x0 = x0; A.x1 = x1; A.w1 = w1; A.b1 = b1;
    A.w_ih0 = w_ih[0]; A.b_ih0 = b_ih[0]; A.b_hh0 = b_hh[0];
    A.w_ih1 = dirs == 2 ? w_ih[1] : nullptr; A.b_ih1 = dirs == 2 ? b_ih[1] : nullptr; A.b_hh1 = dirs == 2 ? b_hh[1] : nullptr;
    if (!A.w_ih0 || !A.b_ih0 || !A.b_hh0 || (dirs == 2 && (!A.w_ih1 || !A.b_ih1 || !A.b_hh1)))
        return fail(PW_EINVAL, "w_ih, b_ih and b_hh: one tensor per direction");
    for (const void *p : {(const void *)x0, (const void *)x1, (const void *)w1, (const void *)b1, (const void *)A.w_ih0,
                          (const void *)A.w_ih1, (const void *)A.b_ih0, (const void *)A.b_ih1, (const void *)A.b_hh0, (const void *)A.b_hh1})
        if (misaligned(p)) return fail(PW_EINVAL, "inputs and parameters must be 4-byte aligned");
    if (misaligned(hid, 16) || misaligned(G, 16)) return fail(PW_EINVAL, "hid and G must be 16-byte aligned");
    A.hid = hid; A.G = G; A.rows = (long)rows; A.d0 = d0; A.d1 = d1; A.dirs = dirs;
    hipLaunchKernelGGL(pw_front_train_forward_kernel, dim3((unsigned)train_split(A.rows).tiles), dim3(kTrainThreads), front_lds(false).bytes,
                       static_cast<hipStream_t>(stream), A);
    PW_HIP_CHECK(hipGetLastError());
    return PW_OK;
}

int pw_front_train_backward(const float *dG, const float *x0, int32_t d0, const float *x1, int32_t d1, const float *hid,
                            const float *w1, const float *const w_ih[2], int64_t rows, int32_t dirs, int32_t H, float *dW1, float *db1,
                            float *const dW_ih[2], float *const db_gate[2], float *dx0, float *dx1, void *scratch,
                            size_t scratch_bytes, void *stream)
{
    if (int rc = front_shape(rows, d0, d1, dirs, H)) return rc;
    if (!dG || !x0 || !hid || !w1 || !w_ih || !dW1 || !db1 || !dW_ih || !db_gate || !scratch) return fail(PW_EINVAL, "null argument");
    if ((x1 != nullptr) != (d1 > 0)) return fail(PW_EINVAL, "x1 comes with d1 > 0 and only then");
    if (dx1 && d1 == 0) return fail(PW_EINVAL, "dx1 comes with d1 > 0 only");
    if (!w_ih[0] || !dW_ih[0] || !db_gate[0] || (dirs == 2 && (!w_ih[1] || !dW_ih[1] || !db_gate[1])))
        return fail(PW_EINVAL, "w_ih, dW_ih and db_gate: one tensor per direction");
    if (scratch_bytes < pw_front_train_scratch_bytes(rows, d0, d1))
        return fail(PW_EINVAL, "scratch_bytes is less than pw_front_train_scratch_bytes(rows, d0, d1)");
    for (const void *p : {(const void *)dG, (const void *)x0, (const void *)x1, (const void *)hid, (const void *)w1, (const void *)w_ih[0],
                          (const void *)(dirs == 2 ? w_ih[1] : nullptr), (const void *)dW1, (const void *)db1, (const void *)dW_ih[0],
                          (const void *)(dirs == 2 ? dW_ih[1] : nullptr), (const void *)db_gate[0],
                          (const void *)(dirs == 2 ? db_gate[1] : nullptr), (const void *)dx0, (const void *)dx1, (const void *)scratch})
        if (misaligned(p)) return fail(PW_EINVAL, "every pointer must be 4-byte aligned");
    const TrainSplit S = train_split((long)rows);
    FrontBwdArgs A;
    A.dG = dG; A.x0 = x0; A.x1 = x1; A.hid = hid; A.w1 = w1; A.w_ih0 = w_ih[0]; A.w_ih1 = dirs == 2 ? w_ih[1] : nullptr;
    A.partial = static_cast<float *>(scratch); A.dx0 = dx0; A.dx1 = dx1;
    A.rows = (long)rows; A.per_group = S.per_group; A.d0 = d0; A.d1 = d1; A.dirs = dirs;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(pw_front_train_backward_kernel, dim3((unsigned)S.groups), dim3(kTrainThreads), front_lds(true).bytes, s, A);
    PW_HIP_CHECK(hipGetLastError());
    FrontReduceArgs R;
    R.partial = A.partial; R.dw_ih0 = dW_ih[0]; R.dw_ih1 = dirs == 2 ? dW_ih[1] : nullptr; R.dw1 = dW1;
    R.db_gate0 = db_gate[0]; R.db_gate1 = dirs == 2 ? db_gate[1] : nullptr; R.db1 = db1;
    R.per_slot = front_partial_floats(d0 + d1); R.groups = S.groups; R.K = d0 + d1; R.dirs = dirs;
    hipLaunchKernelGGL(pw_front_train_reduce_kernel, dim3(train_reduce_blocks(R.per_slot)), dim3(kTrainThreads), 0, s, R);
    PW_HIP_CHECK(hipGetLastError());
    return PW_OK;
}

}  // extern "C"
