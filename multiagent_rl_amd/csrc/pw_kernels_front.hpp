// pw_kernels_front.hpp -- part of libpworld.so (translation unit csrc/pworld_front.hip includes it).
// The dense front of the learner's networks WITH gradient: what all three passes with gradient of an update begin with,
//     [x0 | x1] -> dense1 (Linear(d0 + d1, 64)) -> ReLU -> G = hid W_ih^T + (b_ih + b_hh)      [rows, 256]
// (x0 = the observation rows, x1 = the action rows or nothing; 256 gate columns = 1 x 4 x 64, the critics' LSTM, or 2 x 4 x 32, the
// actor's BiLSTM; G is what pw_lstm_train_forward reads).  pw_front_train_forward_kernel is one launch instead of cat / addmm / relu /
// bias adds / weight cats / addmm; pw_front_train_backward_kernel + pw_front_train_reduce_kernel are two instead of their backward.
//
// Arithmetic: exact float32 on v_mfma_f32_16x16x4_f32 (a chain of fused multiply-adds over its four k, in order).  Orientation of every
// tile, as in the other units: the 16 columns are 16 consecutive ROWS of the batch, the 16 tile rows are output features, so a lane's
// four accumulator registers are four consecutive features of one row and leave as one 16-byte store.
// Long sums are split so that no chain is much longer than 64 terms (a chain's rounding error grows with its length, and a dependent
// chain of matrix instructions also waits for itself): a dot product's k steps go round-robin into 2 or 4 chains that are added as a
// balanced tree at the end; the sums over the rows are pw_train_sums.hpp's.
//
// Forward: a workgroup of four waves owns a tile of 16 rows.  The input rows are staged side by side in LDS (no concatenated copy
// exists in memory; columns up to the next multiple of 8 are zero).  Wave w forms hidden units 16 w .. 16 w + 15 (two chains over the k
// steps of d0 + d1), adds b1, clamps, and leaves them in LDS (and in `hid` when a gradient will need them); after one barrier wave w
// forms gate columns 64 w .. 64 w + 63 (two chains over the 64 hidden units) and adds b_ih + b_hh.  Weights are read where nn.Linear /
// nn.LSTM keep them, one direction's W_ih after the other's: nothing is concatenated.
//
// Backward: the ordered sums of pw_train_sums.hpp (tiles, workgroups, slots, tree; all plain, none compensated).  Per tile: dG,
// [x0 | x1] and hid staged in LDS; dHid = (dG W_ih) o (hid > 0) by wave w for its 16 units (four chains over the 256 gate columns), to
// LDS; then the tile's contribution to dW_ih (= dG^T hid), dW1 (= dHid^T [x0 | x1]) and the two column sums (db_gate, db1) is added
// into the workgroup's registers, and dx = dHid W1 leaves for the columns whose pointer is given.  A slot holds front_partial_floats
// numbers; pw_front_train_reduce_kernel adds the slots and scatters the sums to the six results.  The order of every sum is a
// function of (rows, d0, d1) only.
// Addresses: parameters and inputs are read with 4-byte loads (nn.LSTM's tensors may be views of one flat buffer); hid, G and the
// scratch, which the caller allocates for these launches, are 16-byte aligned.
#pragma once

#include "pw_common.hpp"
#include "pw_lstm_math.hpp"
#include "pw_train_sums.hpp"

namespace {

constexpr int kFrontHid = 64;        // dense1's width = the LSTM's input size
constexpr int kFrontGates = 256;     // dirs * 4 H
constexpr int kFrontMaxD0 = 104, kFrontMaxD1 = 16;
constexpr int kFrontKTiles = 8;      // 16-column tiles of [x0 | x1]: ceil(120 / 16)
constexpr int kFrontXS = train_lds_stride(128), kFrontHS = train_lds_stride(64), kFrontGS = train_lds_stride(256);   // LDS row strides

struct FrontLds { float *xs, *hs, *dgs, *dhs; uint32_t bytes; };
// xs [16][kFrontXS]: [x0 | x1] of the tile's rows; hs [16][kFrontHS]: hid; backward only: dgs [16][kFrontGS]: dG, dhs [16][kFrontHS]: dHid
__host__ __device__ inline FrontLds front_lds(bool backward, unsigned char *raw = nullptr)
{
    LdsCursor c{reinterpret_cast<float *>(raw)}; FrontLds o;
    o.xs = c.take<float>(kTrainTile * kFrontXS, 16); o.hs = c.take<float>(kTrainTile * kFrontHS, 16);
    o.dgs = o.dhs = nullptr;
    if (backward) { o.dgs = c.take<float>(kTrainTile * kFrontGS, 16); o.dhs = c.take<float>(kTrainTile * kFrontHS, 16); }
    o.bytes = 4 * c.at; return o;
}

// one workgroup's partial sums: dW_ih [256][64] (direction 0's rows, then direction 1's), dW1 [64][d0 + d1], db_gate [256], db1 [64]
__host__ __device__ inline long front_partial_floats(int K) { return (long)kFrontGates * kFrontHid + (long)kFrontHid * K + kFrontGates + kFrontHid; }

struct FrontFwdArgs {
    const float *x0, *x1;                 // [rows][d0], [rows][d1] or NULL
    const float *w1, *b1;                 // [64][d0 + d1], [64]
    const float *w_ih0, *w_ih1;           // [4H][64] per direction (w_ih1 unread with one direction)
    const float *b_ih0, *b_ih1, *b_hh0, *b_hh1;
    float *hid, *G;                       // [rows][64] or NULL, [rows][256]
    long rows;
    int d0, d1, dirs;
};

struct FrontBwdArgs {
    const float *dG, *x0, *x1, *hid;      // [rows][256], the forward's inputs, the forward's hid
    const float *w1, *w_ih0, *w_ih1;
    float *partial;                       // [groups][front_partial_floats]
    float *dx0, *dx1;                     // [rows][d0], [rows][d1], each or NULL
    long rows, per_group;
    int d0, d1, dirs;
};

struct FrontReduceArgs {
    const float *partial;
    float *dw_ih0, *dw_ih1, *dw1, *db_gate0, *db_gate1, *db1;
    long per_slot;                        // front_partial_floats
    int groups, K, dirs;
};

// [x0 | x1] of rows r0 .. r0 + 15 -> xs, columns 0 .. width - 1 (width a multiple of 4, <= 128); zero past d0 + d1 and past the last row
__device__ __forceinline__ void front_stage_x(float *xs, const float *__restrict__ x0, const float *__restrict__ x1, const int d0,
                                              const int d1, const long r0, const long rows, const int width, const int tid)
{
    for (int i = tid; i < kTrainTile * width; i += kTrainThreads) {
        const int r = i / width, k = i - r * width;
        float v = 0.0f;
        if (r0 + r < rows) {
            if (k < d0) v = x0[(size_t)(r0 + r) * d0 + k];
            else if (k < d0 + d1) v = x1[(size_t)(r0 + r) * d1 + (k - d0)];
        }
        xs[r * kFrontXS + k] = v;
    }
}

__global__ void __launch_bounds__(kTrainThreads) pw_front_train_forward_kernel(const FrontFwdArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char front_smem[];
    const FrontLds L = front_lds(false, front_smem);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lo = lane & 15, hi = lane >> 4;
    const long r0 = (long)blockIdx.x * kTrainTile;
    const int K = A.d0 + A.d1, kpairs = (K + 7) >> 3;
    const bool row_ok = r0 + lo < A.rows;

    front_stage_x(L.xs, A.x0, A.x1, A.d0, A.d1, r0, A.rows, 8 * kpairs, tid);
    __syncthreads();

    // dense1: units 16 wave .. + 15 of the tile's rows; even and odd k steps in two chains, k ascending in each
    {
        train_f4 even = {0.0f, 0.0f, 0.0f, 0.0f}, odd = {0.0f, 0.0f, 0.0f, 0.0f};
        const float *wrow = A.w1 + (size_t)(16 * wave + lo) * K;
        const float *xrow = L.xs + lo * kFrontXS;
        for (int s = 0; s < kpairs; ++s) {
            const int k = 8 * s + hi;
            even = train_mfma(k < K ? wrow[k] : 0.0f, xrow[k], even);
            odd = train_mfma(k + 4 < K ? wrow[k + 4] : 0.0f, xrow[k + 4], odd);
        }
        const train_f4 acc = even + odd;
        const int u = 16 * wave + 4 * hi;
        float4 h;
        h.x = relu_fwd(acc[0] + A.b1[u + 0]); h.y = relu_fwd(acc[1] + A.b1[u + 1]);
        h.z = relu_fwd(acc[2] + A.b1[u + 2]); h.w = relu_fwd(acc[3] + A.b1[u + 3]);
        *reinterpret_cast<float4 *>(L.hs + lo * kFrontHS + u) = h;
        if (A.hid && row_ok) *reinterpret_cast<float4 *>(A.hid + (size_t)(r0 + lo) * kFrontHid + u) = h;
    }
    __syncthreads();

    // the gate projection: columns 64 wave .. + 63, k ascending over the hidden units
    const int c0 = 64 * wave;
    const bool second = A.dirs == 2 && c0 >= 128;                      // wave-uniform: the reverse direction's rows
    const int g0 = second ? c0 - 128 : c0;                             // first gate row inside the direction's tensors
    const float *w = (second ? A.w_ih1 : A.w_ih0) + (size_t)(g0 + lo) * kFrontHid + hi;
    const float *hrow = L.hs + lo * kFrontHS + hi;
    train_f4 g[4], g_odd[4];                                          // even and odd k steps in two chains, as above
#pragma unroll
    for (int t = 0; t < 4; ++t) g[t] = g_odd[t] = train_f4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int s = 0; s < 16; s += 2) {
        const float b0 = hrow[4 * s], b1 = hrow[4 * s + 4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            g[t] = train_mfma(w[t * 16 * kFrontHid + 4 * s], b0, g[t]);
            g_odd[t] = train_mfma(w[t * 16 * kFrontHid + 4 * s + 4], b1, g_odd[t]);
        }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) g[t] += g_odd[t];
    const float *bi = second ? A.b_ih1 : A.b_ih0, *bh = second ? A.b_hh1 : A.b_hh0;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int q = g0 + 16 * t + 4 * hi;
        float4 o;
        o.x = g[t][0] + (bi[q + 0] + bh[q + 0]); o.y = g[t][1] + (bi[q + 1] + bh[q + 1]);
        o.z = g[t][2] + (bi[q + 2] + bh[q + 2]); o.w = g[t][3] + (bi[q + 3] + bh[q + 3]);
        if (row_ok) *reinterpret_cast<float4 *>(A.G + (size_t)(r0 + lo) * kFrontGates + c0 + 16 * t + 4 * hi) = o;
    }
}

__global__ void __launch_bounds__(kTrainThreads) pw_front_train_backward_kernel(const FrontBwdArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char front_smem[];
    const FrontLds L = front_lds(true, front_smem);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lo = lane & 15, hi = lane >> 4;
    const int K = A.d0 + A.d1, ktiles = (K + 15) >> 4;
    const TrainSplit S = train_split(A.rows);
    const long first = (long)blockIdx.x * A.per_group;
    const long last = first + A.per_group < S.tiles ? first + A.per_group : S.tiles;

    train_f4 dwih[16], dw1[kFrontKTiles];
#pragma unroll
    for (int i = 0; i < 16; ++i) dwih[i] = train_f4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int i = 0; i < kFrontKTiles; ++i) dw1[i] = train_f4{0.0f, 0.0f, 0.0f, 0.0f};
    float gate_sum = 0.0f, hid_sum = 0.0f;   // column tid of dG; column tid of dHid (tid < 64)

    // W_ih^T as the A operand of dHid: row = unit 16 wave + lo, k = gate column
    const float *wt0 = A.w_ih0 + 16 * wave + lo, *wt1 = (A.dirs == 2 ? A.w_ih1 : A.w_ih0 + 128 * kFrontHid) + 16 * wave + lo;

    for (long tile = first; tile < last; ++tile) {
        const long r0 = tile * kTrainTile;
        const bool row_ok = r0 + lo < A.rows;
        front_stage_x(L.xs, A.x0, A.x1, A.d0, A.d1, r0, A.rows, 16 * ktiles, tid);
#pragma unroll
        for (int r = 0; r < kTrainTile; ++r)
            L.dgs[r * kFrontGS + tid] = r0 + r < A.rows ? A.dG[(size_t)(r0 + r) * kFrontGates + tid] : 0.0f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = 4 * i + (tid >> 6), u = tid & 63;
            L.hs[r * kFrontHS + u] = r0 + r < A.rows ? A.hid[(size_t)(r0 + r) * kFrontHid + u] : 0.0f;
        }
        __syncthreads();

        // dHid of units 16 wave .. + 15: k ascending over the gate columns; the ReLU's mask from hid
        {
            train_f4 part[4];                                         // k step s into chain s % 4; (0 + 1) + (2 + 3) at the end
#pragma unroll
            for (int j = 0; j < 4; ++j) part[j] = train_f4{0.0f, 0.0f, 0.0f, 0.0f};
            const float *grow = L.dgs + lo * kFrontGS + hi;
#pragma unroll 2
            for (int s = 0; s < 32; s += 4)
#pragma unroll
                for (int j = 0; j < 4; ++j) part[j] = train_mfma(wt0[(4 * (s + j) + hi) * kFrontHid], grow[4 * (s + j)], part[j]);
#pragma unroll 2
            for (int s = 0; s < 32; s += 4)
#pragma unroll
                for (int j = 0; j < 4; ++j) part[j] = train_mfma(wt1[(4 * (s + j) + hi) * kFrontHid], grow[128 + 4 * (s + j)], part[j]);
            const train_f4 acc = (part[0] + part[1]) + (part[2] + part[3]);
            const int u = 16 * wave + 4 * hi;
            const float4 h = *reinterpret_cast<const float4 *>(L.hs + lo * kFrontHS + u);
            float4 d;
            d.x = h.x > 0.0f ? acc[0] : 0.0f; d.y = h.y > 0.0f ? acc[1] : 0.0f;
            d.z = h.z > 0.0f ? acc[2] : 0.0f; d.w = h.w > 0.0f ? acc[3] : 0.0f;
            *reinterpret_cast<float4 *>(L.dhs + lo * kFrontHS + u) = d;
        }
        gate_sum += train_column_sum(L.dgs + tid, kFrontGS);
        __syncthreads();

        // the tile's 16 rows into the parameter gradients, rows ascending (four k steps of four rows)
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int r = 4 * s + hi;
            float a[4], b[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) { a[t] = L.dgs[r * kFrontGS + 64 * wave + 16 * t + lo]; b[t] = L.hs[r * kFrontHS + 16 * t + lo]; }
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int v = 0; v < 4; ++v) dwih[4 * t + v] = train_mfma(a[t], b[v], dwih[4 * t + v]);
            const float dh = L.dhs[r * kFrontHS + 16 * wave + lo];
#pragma unroll
            for (int j = 0; j < kFrontKTiles; ++j)
                if (j < ktiles) dw1[j] = train_mfma(dh, L.xs[r * kFrontXS + 16 * j + lo], dw1[j]);
        }
        if (tid < kFrontHid) hid_sum += train_column_sum(L.dhs + tid, kFrontHS);

        // dx = dHid W1 for the columns asked for: k tile j by wave j % 4, k ascending over the hidden units
        if (A.dx0 || A.dx1) {
            for (int j = wave; j < ktiles; j += 4) {
                if (!A.dx0 && 16 * j + 16 <= A.d0) continue;          // a tile of x0's columns alone
                if (!A.dx1 && 16 * j >= A.d0) continue;               // a tile of x1's columns alone
                const int kk = 16 * j + lo;
                const float *wcol = A.w1 + (kk < K ? kk : 0);
                const float *drow = L.dhs + lo * kFrontHS + hi;
                train_f4 even = {0.0f, 0.0f, 0.0f, 0.0f}, odd = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 2
                for (int s = 0; s < 16; s += 2) {
                    const float w0 = wcol[(size_t)(4 * s + hi) * K], w4 = wcol[(size_t)(4 * s + 4 + hi) * K];
                    even = train_mfma(kk < K ? w0 : 0.0f, drow[4 * s], even);
                    odd = train_mfma(kk < K ? w4 : 0.0f, drow[4 * s + 4], odd);
                }
                const train_f4 acc = even + odd;
                if (row_ok) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int k = 16 * j + 4 * hi + i;
                        if (k < A.d0) { if (A.dx0) A.dx0[(size_t)(r0 + lo) * A.d0 + k] = acc[i]; }
                        else if (k < K) { if (A.dx1) A.dx1[(size_t)(r0 + lo) * A.d1 + (k - A.d0)] = acc[i]; }
                    }
                }
            }
        }
        __syncthreads();
    }

    // this workgroup's partial sums -> its slot
    float *P = A.partial + (size_t)blockIdx.x * front_partial_floats(K);
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int v = 0; v < 4; ++v)
#pragma unroll
            for (int i = 0; i < 4; ++i) P[(64 * wave + 16 * t + 4 * hi + i) * kFrontHid + 16 * v + lo] = dwih[4 * t + v][i];
    float *P1 = P + kFrontGates * kFrontHid;
#pragma unroll
    for (int j = 0; j < kFrontKTiles; ++j) {
        const int k = 16 * j + lo;
        if (k < K) {
#pragma unroll
            for (int i = 0; i < 4; ++i) P1[(16 * wave + 4 * hi + i) * K + k] = dw1[j][i];
        }
    }
    float *P2 = P1 + kFrontHid * K;
    P2[tid] = gate_sum;
    if (tid < kFrontHid) P2[kFrontGates + tid] = hid_sum;
}

// element e of the parameter gradients = the sum of element e of every slot
__global__ void __launch_bounds__(kTrainThreads) pw_front_train_reduce_kernel(const FrontReduceArgs A)
{
    const long e = (long)blockIdx.x * kTrainThreads + threadIdx.x;
    if (e >= A.per_slot) return;
    const float sum = train_slot_sum(A.partial + e, A.groups, A.per_slot);
    const long n_ih = (long)kFrontGates * kFrontHid, n_w1 = (long)kFrontHid * A.K;
    if (e < n_ih) {
        if (A.dirs == 2 && e >= n_ih / 2) A.dw_ih1[e - n_ih / 2] = sum;
        else A.dw_ih0[e] = sum;
    } else if (e < n_ih + n_w1) {
        A.dw1[e - n_ih] = sum;
    } else if (e < n_ih + n_w1 + kFrontGates) {
        const long c = e - n_ih - n_w1;
        if (A.dirs == 2 && c >= kFrontGates / 2) A.db_gate1[c - kFrontGates / 2] = sum;
        else A.db_gate0[c] = sum;
    } else {
        A.db1[e - n_ih - n_w1 - kFrontGates] = sum;
    }
}

}  // namespace
