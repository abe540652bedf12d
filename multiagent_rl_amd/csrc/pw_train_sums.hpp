// pw_train_sums.hpp -- part of libpworld.so: the ordered sums of the learner's gradient kernels, shared by the dense front
// (pw_kernels_front.hpp), the recurrent-weight gradients (pw_kernels_lstm_wgrad.hpp) and the output layers (pw_kernels_head.hpp).
// No kernel is defined here.
//
// The scheme.  A parameter gradient is a sum over the batch's rows.  The rows are cut into TILES of 16 (the columns of the matrix
// instruction).  train_split hands the tiles to at most kTrainSlots WORKGROUPS of 256 threads: workgroup g owns tiles
// g T .. g T + T - 1, and T and the number of workgroups follow from `rows` alone.  A workgroup adds its tiles, rows ascending, into
// registers that live across them (a tile's 16 rows of a column sum as a balanced tree: train_column_sum), and at the end stores its
// partial sums to its SLOT of the caller's scratch ([groups][per_slot] floats, train_scratch_bytes).  A second kernel of the family,
// one thread per element (train_reduce_blocks workgroups), then adds the slots of every element as a balanced TREE over the
// kTrainSlots slot numbers, slots 2 i and 2 i + 1 first (train_slot_sum); a slot past `groups` is not read and counts as +0.0.  There is
// no floating-point atomic anywhere, and the order of every sum is a function of the shape alone: the same inputs give the same bits
// on every launch, eager or replayed from a graph.  Host and kernel both call train_split, so they cannot disagree.
//
// Compensation.  The output layers' column sums db and their tree over the slots are COMPENSATED (train_two_sum pairs: every
// addition's rounding error is carried beside the sum and added at the end; train_column_sum_comp, and the slot tree at the end of
// pw_kernels_head.hpp, which is train_slot_sum with a train_two_sum in place of every addition and hi + lo as its result): a bias
// gradient is one sum of `rows` numbers of either sign, and when it nearly cancels (a Q head's dOut of mean zero) a plain float32 sum
// keeps the rounding of its large partial sums, several times one rounding of the small result -- measured: 5.8 times at rows = 65 --
// whatever the order.  The pairs cost six additions per element on a few hundred columns.  The dense front's column sums and the
// recurrent-weight gradients use the plain trees.
#pragma once

#include "pw_common.hpp"

namespace {

constexpr int kTrainTile = 16;       // rows per tile = the columns of the matrix instruction
constexpr int kTrainThreads = 256;   // four waves
constexpr int kTrainSlots = 128;     // the most workgroups (= partial sums per element) of one launch

typedef float train_f4 __attribute__((ext_vector_type(4)));

// one step of v_mfma_f32_16x16x4_f32: exact float32, a chain of fused multiply-adds over its four k, in order
__device__ __forceinline__ train_f4 train_mfma(const float a, const float b, const train_f4 acc)
{
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
}

// The LDS row stride, in words, of a staged tile `cols` wide (cols a multiple of 4): the least stride >= cols + 4 that is 20 mod 32.
// A tile is read both along its rows (B operand: lane = row) and across them (A operand: lane = column), and this residue keeps
// both to at most three lanes per bank; a multiple of 4 for the 16-byte writes.
constexpr int train_lds_stride(int cols) { return cols + (20 - cols % 32 + 32) % 32; }

// How a launch splits `rows`: T tiles per workgroup, `groups` workgroups; the summation order follows from it
struct TrainSplit { long tiles; long per_group; int groups; };
__host__ __device__ inline TrainSplit train_split(long rows)
{
    TrainSplit s;
    s.tiles = (rows + kTrainTile - 1) / kTrainTile;
    s.per_group = (s.tiles + kTrainSlots - 1) / kTrainSlots;
    s.groups = (int)((s.tiles + s.per_group - 1) / s.per_group);
    return s;
}
// Host side.  The caller's scratch for that split: one slot of per_slot floats per workgroup
inline size_t train_scratch_bytes(long rows, size_t per_slot) { return sizeof(float) * (size_t)train_split(rows).groups * per_slot; }
// the grid of the kernel that adds the slots: one thread per element of a slot
inline unsigned train_reduce_blocks(long per_slot) { return (unsigned)((per_slot + kTrainThreads - 1) / kTrainThreads); }
// why a launch with one workgroup per tile (a forward) cannot take `rows`, or NULL
inline const char *train_rows_refused(long long rows)
{
    if (rows < 1) return "rows must be >= 1";
    if (rows > (long long)0x7fffffff * kTrainTile) return "rows: more rows than one launch's grid holds";
    return nullptr;
}

// (hi, lo) += (b_hi, b_lo): the rounding error of hi + b_hi (Knuth's two-sum, exact without fused contraction or reassociation --
// the units are compiled with -ffp-contract=off -fno-fast-math) is kept in lo.  The value is hi + lo.
__device__ __forceinline__ void train_two_sum(float &hi, float &lo, const float b_hi, const float b_lo)
{
    const float s = hi + b_hi, bb = s - hi;
    const float err = (hi - (s - bb)) + (b_hi - bb);
    hi = s;
    lo = (lo + b_lo) + err;
}

// the sum of a tile's 16 rows of one column, as a balanced tree (rows 2 i and 2 i + 1 first)
__device__ __forceinline__ float train_column_sum(const float *col, const int stride)
{
    float v[kTrainTile];
#pragma unroll
    for (int r = 0; r < kTrainTile; ++r) v[r] = col[r * stride];
#pragma unroll
    for (int n = kTrainTile / 2; n >= 1; n >>= 1)
#pragma unroll
        for (int i = 0; i < n; ++i) v[i] = v[2 * i] + v[2 * i + 1];
    return v[0];
}

// (hi, lo) += the same sum as a balanced tree of two-sums
__device__ __forceinline__ void train_column_sum_comp(float &hi, float &lo, const float *col, const int stride)
{
    float v[kTrainTile], e[kTrainTile];
#pragma unroll
    for (int r = 0; r < kTrainTile; ++r) { v[r] = col[r * stride]; e[r] = 0.0f; }
#pragma unroll
    for (int n = kTrainTile / 2; n >= 1; n >>= 1)
#pragma unroll
        for (int i = 0; i < n; ++i) {
            float h = v[2 * i], l = e[2 * i];
            train_two_sum(h, l, v[2 * i + 1], e[2 * i + 1]);
            v[i] = h; e[i] = l;
        }
    train_two_sum(hi, lo, v[0], e[0]);
}

// the sum of one element (p: its place in slot 0) over the slots, as a balanced tree over the kTrainSlots slot numbers
__device__ __forceinline__ float train_slot_sum(const float *p, const int groups, const long per_slot)
{
    float c[kTrainSlots / 8];
#pragma unroll
    for (int i = 0; i < kTrainSlots / 8; ++i) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = 8 * i + j < groups ? p[(size_t)(8 * i + j) * per_slot] : 0.0f;
        c[i] = ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
    }
#pragma unroll
    for (int n = kTrainSlots / 16; n >= 1; n >>= 1)
#pragma unroll
        for (int i = 0; i < n; ++i) c[i] = c[2 * i] + c[2 * i + 1];
    return c[0];
}

// The same tree over two-sum pairs is the one piece that is NOT here: its body stands in pw_head_train_reduce_kernel
// (pw_kernels_head.hpp), its only user, and calls train_two_sum.  As a function of this header it costs that kernel registers in
// every form tried: forced inline 256 VGPR + 133 AGPR against the 256 + 8 of the body in place; `inline`, with the pointers by value,
// by reference, __restrict__, or the lo pointer formed inside, 256 + 13.  A second kernel that needs it should move it here and
// look at both kernels' registers (tools/train_sums_codegen.py).

}  // namespace
