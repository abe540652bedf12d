// pw_kernels_lstm_wgrad.hpp -- part of libpworld.so (translation unit csrc/pworld_lstm_wgrad.hip includes it).
// dW_hh of the learner's LSTMs: the two recurrent-weight gradients, dG^T against the direction's PREVIOUS output, from dG as
// pw_lstm_train_backward_kernel writes it and Y as pw_lstm_train_forward_kernel writes it (pw_kernels_lstm.hpp), both read in place:
//     dw_fw[r][k] = sum over (seq, t = 1 .. N - 1) of dG[seq][t][0][r] Y[seq][t - 1][k]
//     dw_bw[r][k] = sum over (seq, t = 0 .. N - 2) of dG[seq][t][1][r] Y[seq][t + 1][H + k]            (r < 4 H, k < H)
// Exact float32 on v_mfma_f32_16x16x4_f32, laid out as the dense front's dW_ih (pw_kernels_front.hpp), summed by the ordered sums of
// pw_train_sums.hpp (plain, not compensated): the flat rows (seq, t) are cut into tiles of 16 without regard to sequence ends, and P
// below is a workgroup's number of tiles.  Per tile the 256 gate columns of dG and the 64 columns of the
// SHIFTED Y row (row - 1 under direction 0's columns, row + 1 under direction 1's) are staged in LDS.  A row that has no previous step
// in its direction (t = 0 forward, t = N - 1 reverse) or lies past the last sequence is staged as zeros on BOTH sides by a select: its
// dG is never multiplied, so a NaN there stays out of the sums, and the shifted row of a live (row, direction) is always a row of the
// same sequence.  Wave w owns gate columns 64 w .. 64 w + 63 (with two directions: waves 0, 1 direction 0, waves 2, 3 direction 1,
// against that direction's 32 columns of Y); a tile is four matrix steps of four rows, rows ascending, steps 0 and 2 into one
// accumulator chain and 1 and 3 into another (kept in registers across the workgroup's tiles, added at the end), so a chain is
// 2 P steps long.  A slot holds [4 H][H] per direction, direction 0 first; pw_lstm_train_wgrad_reduce_kernel adds the slots.  The
// order of every sum is a function of (b, N, dirs) alone.  A direction whose output is not asked for is neither multiplied nor
// stored nor reduced.
#pragma once

#include "pw_common.hpp"
#include "pw_train_sums.hpp"

namespace {

constexpr int kLstmWgradCols = 256, kLstmWgradYCols = 64;                   // dirs * 4 H, dirs * H: the same for both shapes
constexpr int kLstmWgradGS = train_lds_stride(kLstmWgradCols), kLstmWgradYS = train_lds_stride(kLstmWgradYCols);   // LDS row strides
constexpr int kLstmWgradSlot = kLstmWgradCols * kLstmWgradYCols;            // floats of one slot at dirs = 1; half of it at dirs = 2

__host__ __device__ inline long lstm_wgrad_slot_floats(int dirs) { return kLstmWgradSlot / dirs; }

struct LstmWgradLds { float *dgs, *ys; uint32_t bytes; };
__host__ __device__ inline LstmWgradLds lstm_wgrad_lds(unsigned char *raw = nullptr)
{
    LdsCursor c{reinterpret_cast<float *>(raw)}; LstmWgradLds o;
    o.dgs = c.take<float>(kTrainTile * kLstmWgradGS, 16); o.ys = c.take<float>(kTrainTile * kLstmWgradYS, 16);
    o.bytes = 4 * c.at; return o;
}

// dG [b][N][DIRS][4 H], Y [b][N][DIRS H] -> partial [groups][lstm_wgrad_slot_floats]; want: bit d set = direction d is asked for
template <int H, int DIRS>
__global__ void __launch_bounds__(kTrainThreads) pw_lstm_train_wgrad_kernel(const float *__restrict__ dG, const float *__restrict__ Y,
                                                                           const long rows, const int N, const long per_group,
                                                                           const int want, float *__restrict__ partial)
{
    static_assert(DIRS * 4 * H == kLstmWgradCols && DIRS * H == kLstmWgradYCols, "256 gate columns against 64 output columns");
    extern __shared__ __attribute__((aligned(16))) unsigned char lstm_wgrad_smem[];
    const LstmWgradLds L = lstm_wgrad_lds(lstm_wgrad_smem);
    constexpr int V = 4 / DIRS;                                              // 16-column tiles of Y that a wave's direction has
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lo = lane & 15, hi = lane >> 4;
    const int wdir = DIRS == 2 ? wave >> 1 : 0;                              // the direction of this wave's 64 gate columns
    const bool wave_on = (want >> wdir) & 1;
    const int gdir = DIRS == 2 ? tid >> 7 : 0;                               // the direction of gate column tid (staging)
    const int ydir = DIRS == 2 ? (tid & 63) >> 5 : 0;                        // the direction of Y column tid & 63 (staging)
    const TrainSplit S = train_split(rows);
    const long first = (long)blockIdx.x * per_group;
    const long last = first + per_group < S.tiles ? first + per_group : S.tiles;

    train_f4 acc[2][4 * V];
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int i = 0; i < 4 * V; ++i) acc[c][i] = train_f4{0.0f, 0.0f, 0.0f, 0.0f};

    for (long tile = first; tile < last; ++tile) {
        const long r0 = tile * kTrainTile;
        const int t0 = (int)(r0 % N);
#pragma unroll
        for (int r = 0; r < kTrainTile; ++r) {
            const int t = (t0 + r) % N;
            const bool live = r0 + r < rows && ((want >> gdir) & 1) && (gdir ? t < N - 1 : t > 0);
            L.dgs[r * kLstmWgradGS + tid] = live ? dG[(size_t)(r0 + r) * kLstmWgradCols + tid] : 0.0f;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = 4 * i + (tid >> 6), u = tid & 63;
            const int t = (t0 + r) % N;
            const bool live = r0 + r < rows && ((want >> ydir) & 1) && (ydir ? t < N - 1 : t > 0);
            const long src = ydir ? r0 + r + 1 : r0 + r - 1;                 // live: 0 <= src < rows, a row of the same sequence
            L.ys[r * kLstmWgradYS + u] = live ? Y[(size_t)src * kLstmWgradYCols + u] : 0.0f;
        }
        __syncthreads();
        if (wave_on) {
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int r = 4 * s + hi;
                float a[4], y[V];
#pragma unroll
                for (int t = 0; t < 4; ++t) a[t] = L.dgs[r * kLstmWgradGS + 64 * wave + 16 * t + lo];
#pragma unroll
                for (int v = 0; v < V; ++v) y[v] = L.ys[r * kLstmWgradYS + wdir * H + 16 * v + lo];
#pragma unroll
                for (int t = 0; t < 4; ++t)
#pragma unroll
                    for (int v = 0; v < V; ++v)
                        acc[s & 1][V * t + v] = train_mfma(a[t], y[v], acc[s & 1][V * t + v]);
            }
        }
        __syncthreads();
    }

    if (!wave_on) return;
    // this workgroup's sums -> its slot: gate column c = 64 wave + 16 t + 4 hi + i is row c of [DIRS][4 H][H] flattened
    float *P = partial + (size_t)blockIdx.x * lstm_wgrad_slot_floats(DIRS);
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const train_f4 sum = acc[0][V * t + v] + acc[1][V * t + v];
#pragma unroll
            for (int i = 0; i < 4; ++i) P[(64 * wave + 16 * t + 4 * hi + i) * H + 16 * v + lo] = sum[i];
        }
}

// element e of [dw_fw | dw_bw] = the sum of element e of every slot.  An output that is NULL is neither read nor written.
__global__ void __launch_bounds__(kTrainThreads) pw_lstm_train_wgrad_reduce_kernel(const float *__restrict__ partial, const int groups,
                                                                                  const long per_slot, const long per_dir,
                                                                                  float *__restrict__ dw_fw, float *__restrict__ dw_bw)
{
    const long e = (long)blockIdx.x * kTrainThreads + threadIdx.x;
    if (e >= per_slot) return;
    float *out = e < per_dir ? dw_fw : dw_bw;
    if (!out) return;
    out[e < per_dir ? e : e - per_dir] = train_slot_sum(partial + e, groups, per_slot);
}

}  // namespace
