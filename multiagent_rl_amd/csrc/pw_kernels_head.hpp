// pw_kernels_head.hpp -- part of libpworld.so (translation unit csrc/pworld_head.hip includes it).
// The output layers of the learner's networks WITH gradient: what all three passes with gradient of an update end with,
//     A = relu ? max(X, 0) : X;    out_k = A W_k^T + b_k     for k < heads (1 .. 3),   X [rows, 64], W_k [n_k, 64], 1 <= n_k <= 104
// (the actor: the ReLU on the BiLSTM's output and the policy head(s), a third head in the model-learning variant; the critics: one or
// two heads on the pooled context, or the per-step head).  pw_head_train_forward_kernel is one launch instead of relu + an addmm per
// head; pw_head_train_backward_kernel + pw_head_train_reduce_kernel are two instead of two mm and a column sum per head, the adds that
// merge the heads' dX and threshold_backward:
//     dX = (sum_k dOut_k W_k) o (relu ? X > 0 : 1);    dW_k = dOut_k^T A;    db_k = sum over rows of dOut_k.
// The ReLU'd copy A never exists in memory: both kernels form it from X while they stage a tile, and the backward's mask is A > 0.
// A head whose dOut is NULL (it received no gradient) is not in the backward's argument list at all: the host hands the kernel the
// heads that have one, in order, so such a head costs nothing and a launch with only head 0 used is the one-head launch.
//
// Arithmetic: exact float32 on v_mfma_f32_16x16x4_f32 (a chain of fused multiply-adds over its four k, in order), in the orientation
// of the other units: the 16 columns of a tile are 16 consecutive ROWS of the batch, the 16 tile rows are output features.  Why the
// matrix instruction and not plain vector code: its float32 rate equals the vector unit's, and the launches are bound by reading X
// and by launch latency (the widest is 82 MFLOP, the common one 4), so the choice is about registers and code, not speed -- one operand
// register per lane and a 16 x 16 tile per accumulator keep the 21 parameter-gradient tiles of the widest shape in 84 registers, and
// a batch row is a COLUMN of every product, so a non-finite value in row r of X or dOut reaches nothing of another row (idle
// slots of a ragged tile hold zeros in both operands, and no product pairs a row's value with another row's except in dW and db,
// which sum over the rows).
// Long sums are split into short chains that are added as trees: a dot product's k steps go alternately into two chains (even and
// odd steps, k ascending in each) that are added at the end; the heads' contributions to dX are added in head order (a launch's first
// head starts the sum: no zero is added); the sums over the rows are pw_train_sums.hpp's, and here they are the COMPENSATED ones: the
// column sums db as two-sum pairs, and the tree over the slots as two-sum pairs for every element (a dW element's lo part starts at 0).
//
// Forward: a workgroup of four waves owns 64 rows; all stage A (4-byte loads, a lane per column), then wave w forms every head's
// columns for rows 16 w .. 16 w + 15, 16 columns at a time, and adds the bias.  X is read once for all heads.
//
// Backward: the ordered sums of pw_train_sums.hpp (tiles, workgroups, slots, tree).  Per tile of 16 rows: A and every head's dOut
// staged in LDS (a head's columns padded with zeros to a multiple of 16); dX of features 16 w .. 16 w + 15 by wave w; then the tile's
// contribution to dW (for wave w: columns 16 w .. 16 w + 15 of every head's dW, one accumulator per 16 rows of dW) is added into the
// workgroup's registers, and the column sums of dOut likewise.  A slot holds head_partial_floats numbers per head, and
// pw_head_train_reduce_kernel adds the slots -- or, when the split gives ONE workgroup (rows <= 16), the main kernel stores the
// results themselves (hi + lo of a column sum's pair) and no second launch follows.  The order of every sum is a function of
// (rows, the heads' widths) only.
// Addresses: X, dOut, weights, biases and every result are read and written with 4-byte accesses (a parameter may be a view into a
// flat buffer; out_k's rows are n_k numbers long); dX, which the caller allocates for this launch, is 16-byte aligned.
#pragma once

#include "pw_common.hpp"
#include "pw_lstm_math.hpp"
#include "pw_train_sums.hpp"

namespace {

constexpr int kHeadK = 64;            // the width of X = the heads' input size
constexpr int kHeadMaxHeads = 3;
constexpr int kHeadMaxN = 104;        // the widest head
constexpr int kHeadFwdRows = 64;      // rows of one forward workgroup: a tile per wave
constexpr int kHeadMaxColTiles = 21;  // 16-column tiles of all heads: 3 * ceil(104 / 16)
constexpr int kHeadXS = train_lds_stride(kHeadK), kHeadDS = train_lds_stride(16 * kHeadMaxColTiles);   // LDS row strides

struct HeadLds { float *xs, *ds; uint32_t bytes; };
// xs [rows of the workgroup][kHeadXS]: A of the workgroup's rows (forward: 64, backward: 16); backward only: ds [16][kHeadDS]: the
// heads' dOut side by side, head a's columns from 16 * (its first column tile)
__host__ __device__ inline HeadLds head_lds(bool backward, unsigned char *raw = nullptr)
{
    LdsCursor c{reinterpret_cast<float *>(raw)}; HeadLds o;
    o.xs = c.take<float>((backward ? kTrainTile : kHeadFwdRows) * kHeadXS, 16);
    o.ds = nullptr;
    if (backward) o.ds = c.take<float>(kTrainTile * kHeadDS, 16);
    o.bytes = 4 * c.at; return o;
}

// one head's share of a workgroup's partial sums: dW [n][64], then db as two-sum pairs: hi [n], lo [n]
__host__ __device__ inline long head_partial_floats(int n) { return (long)n * kHeadK + 2 * n; }

struct HeadFwdArgs {
    const float *x;                       // [rows][64]
    const float *w[kHeadMaxHeads], *b[kHeadMaxHeads];
    float *out[kHeadMaxHeads];            // [rows][n]
    long rows;
    int n[kHeadMaxHeads];
    int heads, relu;
};

// the heads of a backward launch are those with a dOut, in order
struct HeadBwdArgs {
    const float *x;
    const float *dout[kHeadMaxHeads], *w[kHeadMaxHeads];
    float *dw[kHeadMaxHeads], *db[kHeadMaxHeads];   // where the sums go when the launch has one workgroup
    float *partial;                       // [groups][per_slot] otherwise
    float *dx;                            // [rows][64] or NULL
    long rows, per_group, per_slot;
    int n[kHeadMaxHeads];
    int tile0[kHeadMaxHeads];             // the head's first column tile
    int base[kHeadMaxHeads];              // the head's first number inside a slot
    int heads, relu, ntiles, direct;
};

struct HeadReduceArgs {
    const float *partial;
    float *dw[kHeadMaxHeads], *db[kHeadMaxHeads];
    long per_slot;
    int n[kHeadMaxHeads], base[kHeadMaxHeads];
    int heads, groups;
};

// A of rows r0 .. r0 + count - 1 -> xs; zero past the last row
__device__ __forceinline__ void head_stage_x(float *xs, const float *__restrict__ x, const long r0, const long rows, const int count,
                                             const int relu, const int tid)
{
    for (int i = tid; i < count * kHeadK; i += kTrainThreads) {
        const int r = i >> 6, k = i & 63;
        float v = 0.0f;
        if (r0 + r < rows) v = x[(size_t)(r0 + r) * kHeadK + k];
        xs[r * kHeadXS + k] = relu ? relu_fwd(v) : v;
    }
}

__global__ void __launch_bounds__(kTrainThreads) pw_head_train_forward_kernel(const HeadFwdArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char head_smem[];
    const HeadLds L = head_lds(false, head_smem);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lo = lane & 15, hi = lane >> 4;
    const long r0 = (long)blockIdx.x * kHeadFwdRows;

    head_stage_x(L.xs, A.x, r0, A.rows, kHeadFwdRows, A.relu, tid);
    __syncthreads();

    const long row = r0 + kTrainTile * wave + lo;                      // this lane's row: a column of every tile
    if (r0 + kTrainTile * wave >= A.rows) return;                      // wave-uniform: a tile past the last row
    const bool row_ok = row < A.rows;
    float xb[16];                                                     // the row's 64 numbers, k = 4 s + hi
    const float *xrow = L.xs + (kTrainTile * wave + lo) * kHeadXS + hi;
#pragma unroll
    for (int s = 0; s < 16; ++s) xb[s] = xrow[4 * s];

#pragma unroll
    for (int k = 0; k < kHeadMaxHeads; ++k) {
        if (k >= A.heads) break;
        const int n = A.n[k];
        const float *__restrict__ w = A.w[k], *__restrict__ b = A.b[k];
        float *__restrict__ out = A.out[k];
        for (int c0 = 0; c0 < n; c0 += kTrainTile) {
            const int j = c0 + lo;                                    // the output column whose weights this lane feeds
            const float *wrow = w + (size_t)(j < n ? j : 0) * kHeadK + hi;
            train_f4 even = {0.0f, 0.0f, 0.0f, 0.0f}, odd = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int s = 0; s < 16; s += 2) {
                const float w0 = wrow[4 * s], w4 = wrow[4 * s + 4];
                even = train_mfma(j < n ? w0 : 0.0f, xb[s], even);
                odd = train_mfma(j < n ? w4 : 0.0f, xb[s + 1], odd);
            }
            const train_f4 acc = even + odd;
            if (row_ok) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int c = c0 + 4 * hi + i;
                    if (c < n) out[(size_t)row * n + c] = acc[i] + b[c];
                }
            }
        }
    }
}

__global__ void __launch_bounds__(kTrainThreads) pw_head_train_backward_kernel(const HeadBwdArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char head_smem[];
    const HeadLds L = head_lds(true, head_smem);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lo = lane & 15, hi = lane >> 4;
    const TrainSplit S = train_split(A.rows);
    const long first = (long)blockIdx.x * A.per_group;
    const long last = first + A.per_group < S.tiles ? first + A.per_group : S.tiles;
    const int cols = kTrainTile * A.ntiles;                            // the staged columns of dOut, padding included

    train_f4 dw[kHeadMaxColTiles];                                     // rows 16 t .. + 15 (t a column tile of dOut), columns 16 wave .. + 15 of dW
#pragma unroll
    for (int t = 0; t < kHeadMaxColTiles; ++t) dw[t] = train_f4{0.0f, 0.0f, 0.0f, 0.0f};
    float col_hi0 = 0.0f, col_lo0 = 0.0f, col_hi1 = 0.0f, col_lo1 = 0.0f;   // staged columns tid and tid + 256 of dOut, as two-sum pairs

    for (long tile = first; tile < last; ++tile) {
        const long r0 = tile * kTrainTile;
        head_stage_x(L.xs, A.x, r0, A.rows, kTrainTile, A.relu, tid);
#pragma unroll
        for (int a = 0; a < kHeadMaxHeads; ++a) {
            if (a >= A.heads) break;
            const int n = A.n[a], width = ((n + kTrainTile - 1) / kTrainTile) * kTrainTile;
            const float *__restrict__ d = A.dout[a];
            float *dst = L.ds + kTrainTile * A.tile0[a];
            for (int i = tid; i < kTrainTile * width; i += kTrainThreads) {
                const int r = i / width, c = i - r * width;
                dst[r * kHeadDS + c] = (r0 + r < A.rows && c < n) ? d[(size_t)(r0 + r) * n + c] : 0.0f;
            }
        }
        __syncthreads();

        // dX of features 16 wave .. + 15: per head two chains over its columns (k ascending), the heads added in order
        if (A.dx) {
            train_f4 sum = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int a = 0; a < kHeadMaxHeads; ++a) {
                if (a >= A.heads) break;
                const int n = A.n[a];
                const float *wcol = A.w[a] + kTrainTile * wave + lo;   // W^T as the A operand: row = feature, k = the head's column
                const float *drow = L.ds + lo * kHeadDS + kTrainTile * A.tile0[a] + hi;
                train_f4 even = {0.0f, 0.0f, 0.0f, 0.0f}, odd = {0.0f, 0.0f, 0.0f, 0.0f};
                for (int j0 = 0; j0 < n; j0 += 8) {                   // the padding to 16 columns holds zeros
                    const int j = j0 + hi;
                    const float w0 = wcol[(size_t)(j < n ? j : 0) * kHeadK], w4 = wcol[(size_t)(j + 4 < n ? j + 4 : 0) * kHeadK];
                    even = train_mfma(j < n ? w0 : 0.0f, drow[j0], even);
                    odd = train_mfma(j + 4 < n ? w4 : 0.0f, drow[j0 + 4], odd);
                }
                const train_f4 part = even + odd;
                sum = a == 0 ? part : sum + part;
            }
            const int u = kTrainTile * wave + 4 * hi;
            if (A.relu) {
                const float4 h = *reinterpret_cast<const float4 *>(L.xs + lo * kHeadXS + u);
                sum[0] = h.x > 0.0f ? sum[0] : 0.0f; sum[1] = h.y > 0.0f ? sum[1] : 0.0f;
                sum[2] = h.z > 0.0f ? sum[2] : 0.0f; sum[3] = h.w > 0.0f ? sum[3] : 0.0f;
            }
            if (r0 + lo < A.rows) {
                float4 o; o.x = sum[0]; o.y = sum[1]; o.z = sum[2]; o.w = sum[3];
                *reinterpret_cast<float4 *>(A.dx + (size_t)(r0 + lo) * kHeadK + u) = o;
            }
        }

        // the tile's 16 rows into dW, rows ascending (four k steps of four rows)
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int r = 4 * s + hi;
            const float b = L.xs[r * kHeadXS + kTrainTile * wave + lo];
            const float *drow = L.ds + r * kHeadDS + lo;
#pragma unroll
            for (int t = 0; t < kHeadMaxColTiles; ++t)
                if (t < A.ntiles) dw[t] = train_mfma(drow[kTrainTile * t], b, dw[t]);
        }
        if (tid < cols) train_column_sum_comp(col_hi0, col_lo0, L.ds + tid, kHeadDS);
        if (tid + kTrainThreads < cols) train_column_sum_comp(col_hi1, col_lo1, L.ds + tid + kTrainThreads, kHeadDS);
        __syncthreads();
    }

    // this workgroup's sums -> its slot, or the results themselves when it is the only one
    float *P = A.partial + (size_t)blockIdx.x * A.per_slot;
#pragma unroll
    for (int t = 0; t < kHeadMaxColTiles; ++t) {
        if (t < A.ntiles) {
            const int a = (A.heads > 1 && t >= A.tile0[1]) + (A.heads > 2 && t >= A.tile0[2]);
            const int n = a == 0 ? A.n[0] : a == 1 ? A.n[1] : A.n[2];
            const int t0 = a == 0 ? A.tile0[0] : a == 1 ? A.tile0[1] : A.tile0[2];
            float *to = A.direct ? (a == 0 ? A.dw[0] : a == 1 ? A.dw[1] : A.dw[2]) : P + (a == 0 ? A.base[0] : a == 1 ? A.base[1] : A.base[2]);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int j = kTrainTile * (t - t0) + 4 * hi + i;
                if (j < n) to[(size_t)j * kHeadK + kTrainTile * wave + lo] = dw[t][i];
            }
        }
    }
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const int c = tid + half * kTrainThreads;
        if (c < cols) {
            const int t = c >> 4;
            const int a = (A.heads > 1 && t >= A.tile0[1]) + (A.heads > 2 && t >= A.tile0[2]);
            const int n = a == 0 ? A.n[0] : a == 1 ? A.n[1] : A.n[2];
            const int j = c - kTrainTile * (a == 0 ? A.tile0[0] : a == 1 ? A.tile0[1] : A.tile0[2]);
            float *to = A.direct ? (a == 0 ? A.db[0] : a == 1 ? A.db[1] : A.db[2])
                                 : P + (a == 0 ? A.base[0] : a == 1 ? A.base[1] : A.base[2]) + (size_t)n * kHeadK;
            const float hi_sum = half ? col_hi1 : col_hi0, lo_sum = half ? col_lo1 : col_lo0;
            if (j < n) {
                if (A.direct) to[j] = hi_sum + lo_sum;
                else { to[j] = hi_sum; to[n + j] = lo_sum; }
            }
        }
    }
}

// element e of the parameter gradients = the sum of element e of every slot
__global__ void __launch_bounds__(kTrainThreads) pw_head_train_reduce_kernel(const HeadReduceArgs A)
{
    const long e = (long)blockIdx.x * kTrainThreads + threadIdx.x;
    if (e >= A.per_slot) return;
    const int a = (A.heads > 1 && e >= A.base[1]) + (A.heads > 2 && e >= A.base[2]);
    const int n = a == 0 ? A.n[0] : a == 1 ? A.n[1] : A.n[2];
    const long off = e - (a == 0 ? A.base[0] : a == 1 ? A.base[1] : A.base[2]);
    const long n_w = (long)n * kHeadK;
    if (off >= n_w + n) return;                                       // the lo half of a db pair: its hi thread reads it
    const bool pair = off >= n_w;
    const float *p = A.partial + e, *q = p + (pair ? n : 0);
    // train_slot_sum's tree (pw_train_sums.hpp, which says why this body is here and not there) over two-sum pairs: the hi parts at p,
    // the lo parts at q when `pair` (else they count as zero)
    float c[kTrainSlots / 8], d[kTrainSlots / 8];
#pragma unroll
    for (int i = 0; i < kTrainSlots / 8; ++i) {
        float v[8], w[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const bool in = 8 * i + j < A.groups;
            v[j] = in ? p[(size_t)(8 * i + j) * A.per_slot] : 0.0f;
            w[j] = in && pair ? q[(size_t)(8 * i + j) * A.per_slot] : 0.0f;
        }
#pragma unroll
        for (int m = 4; m >= 1; m >>= 1)
#pragma unroll
            for (int j = 0; j < m; ++j) {
                float h = v[2 * j], l = w[2 * j];
                train_two_sum(h, l, v[2 * j + 1], w[2 * j + 1]);
                v[j] = h; w[j] = l;
            }
        c[i] = v[0]; d[i] = w[0];
    }
#pragma unroll
    for (int m = kTrainSlots / 16; m >= 1; m >>= 1)
#pragma unroll
        for (int i = 0; i < m; ++i) {
            float h = c[2 * i], l = d[2 * i];
            train_two_sum(h, l, c[2 * i + 1], d[2 * i + 1]);
            c[i] = h; d[i] = l;
        }
    const float sum = c[0] + d[0];
    float *dw = a == 0 ? A.dw[0] : a == 1 ? A.dw[1] : A.dw[2], *db = a == 0 ? A.db[0] : a == 1 ? A.db[1] : A.db[2];
    if (pair) db[off - n_w] = sum;
    else dw[off] = sum;
}

}  // namespace
