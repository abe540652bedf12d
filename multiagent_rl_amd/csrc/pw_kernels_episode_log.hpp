// pw_kernels_episode_log.hpp -- part of libpworld.so: the kernels of pw_episode_log_absorb (include/pworld.h has the contract).
//
// One chunk's rew [T,B,N] float32 and terminal [T,B] uint8 -> one log entry per finished episode, in row-major order of the set flags.
// Four launches on one stream, no atomic of any kind:
//   1. pw_episode_log_count_kernel   one workgroup per TILE of kLogTile consecutive flags (flat index i = t B + e): the tile's number of
//                                    set flags -> tile_count[tile];
//   2. pw_episode_log_offsets_kernel one workgroup: tile_count -> its exclusive prefix sum, in place; then the cells: the header keeps
//                                    *length and *step_base as they stood (the walk's bases) and the cells advance by the chunk's
//                                    finished episodes and by T;
//   3. pw_episode_log_slots_kernel   one workgroup per tile: slot[i] = tile offset + the flags before i inside the tile, for every i;
//   4. pw_episode_log_walk_kernel    one thread per running sum, T steps each: threads [0, B N) own by_agent column (e, a) -- thread g
//                                    reads rew[t B N + g], so a wave reads 64 consecutive floats per step -- and threads [B N, B N + B)
//                                    own env e's total, N additions per step in agent order.  Where terminal[t,e] is set the thread
//                                    stores its sum at slot (if below capacity) and ASSIGNS +0.0.  One accumulator per thread, in a
//                                    register: no array indexed at run time.
// Integer sums only cross threads (the prefix sums); every float64 sum is one thread's chain in the order of experiments/run.py:55-57.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

constexpr int kLogThreads = 256;                 // every kernel of this unit
constexpr int kLogPerThread = 4;                 // consecutive flags one thread of the count / slot kernels owns
constexpr int kLogTile = kLogThreads * kLogPerThread;

// what the offsets kernel leaves for the walk: the cells as they stood before this chunk
struct EpisodeLogHeader {
    long long length0;
    long long step0;
};

// The flags [i0, i0 + 4) of this thread (0 past the end) -> their number; f[j] = flag j as 0 / 1.
__device__ __forceinline__ int log_load_flags(const uint8_t *__restrict__ terminal, long long total, long long i0, int f[kLogPerThread])
{
    int n = 0;
#pragma unroll
    for (int j = 0; j < kLogPerThread; ++j) {
        f[j] = (i0 + j < total && terminal[i0 + j] != 0) ? 1 : 0;
        n += f[j];
    }
    return n;
}

// Inclusive prefix sum of one int per thread over the workgroup (Hillis-Steele in LDS, buf holds kLogThreads ints); every thread gets
// its inclusive sum.  Ends with a barrier: buf may be reused at once.
__device__ __forceinline__ int log_block_inclusive_scan(int v, int *buf)
{
    const int tid = threadIdx.x;
    buf[tid] = v;
    __syncthreads();
#pragma unroll
    for (int d = 1; d < kLogThreads; d <<= 1) {
        const int add = tid >= d ? buf[tid - d] : 0;
        __syncthreads();
        buf[tid] += add;
        __syncthreads();
    }
    const int inc = buf[tid];
    __syncthreads();
    return inc;
}

__global__ void __launch_bounds__(kLogThreads) pw_episode_log_count_kernel(const uint8_t *__restrict__ terminal, long long total,
                                                                           int *__restrict__ tile_count)
{
    __shared__ int buf[kLogThreads];
    int f[kLogPerThread];
    const long long i0 = ((long long)blockIdx.x * kLogThreads + threadIdx.x) * kLogPerThread;
    const int inc = log_block_inclusive_scan(log_load_flags(terminal, total, i0, f), buf);
    if (threadIdx.x == kLogThreads - 1) tile_count[blockIdx.x] = inc;
}

__global__ void __launch_bounds__(kLogThreads) pw_episode_log_offsets_kernel(int *__restrict__ tile_count, int tiles, int T,
                                                                             long long *__restrict__ length,
                                                                             long long *__restrict__ step_base,
                                                                             EpisodeLogHeader *__restrict__ header)
{
    __shared__ int buf[kLogThreads];
    __shared__ int last;
    int before = 0;                               // flags in the tiles behind this pass (<= T B < 2^31)
    for (int base = 0; base < tiles; base += kLogThreads) {
        const int i = base + threadIdx.x;
        const int v = i < tiles ? tile_count[i] : 0;
        const int inc = log_block_inclusive_scan(v, buf);
        if (i < tiles) tile_count[i] = before + inc - v;
        if (threadIdx.x == kLogThreads - 1) last = inc;
        __syncthreads();
        before += last;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const long long l0 = *length, s0 = *step_base;
        header->length0 = l0;
        header->step0 = s0;
        *length = l0 + before;
        *step_base = s0 + T;
    }
}

__global__ void __launch_bounds__(kLogThreads) pw_episode_log_slots_kernel(const uint8_t *__restrict__ terminal, long long total,
                                                                           const int *__restrict__ tile_offset, int *__restrict__ slot)
{
    __shared__ int buf[kLogThreads];
    int f[kLogPerThread];
    const long long i0 = ((long long)blockIdx.x * kLogThreads + threadIdx.x) * kLogPerThread;
    const int n = log_load_flags(terminal, total, i0, f);
    int k = tile_offset[blockIdx.x] + log_block_inclusive_scan(n, buf) - n;
#pragma unroll
    for (int j = 0; j < kLogPerThread; ++j) {
        if (i0 + j < total) slot[i0 + j] = k;
        k += f[j];
    }
}

__global__ void __launch_bounds__(kLogThreads) pw_episode_log_walk_kernel(
    const float *__restrict__ rew, const uint8_t *__restrict__ terminal, const int *__restrict__ slot,
    const EpisodeLogHeader *__restrict__ header, int T, int B, int N, long long capacity, double *__restrict__ total,
    double *__restrict__ by_agent, long long *__restrict__ end_step, int *__restrict__ env, double *__restrict__ carry)
{
    const long long g = (long long)blockIdx.x * kLogThreads + threadIdx.x;
    const long long shares = (long long)B * N;
    if (g >= shares + B) return;
    const long long length0 = header->length0, step0 = header->step0;
    if (g < shares) {                              // agent a's share of env e's episode
        const int e = (int)(g / N), a = (int)(g - (long long)e * N);
        double acc = carry[(long long)e * (N + 1) + a];
        const float *r = rew + g;
        const uint8_t *f = terminal + e;
        const int *s = slot + e;
#pragma unroll 4
        for (int t = 0; t < T; ++t) {
            acc += (double)r[(long long)t * shares];
            if (f[(long long)t * B]) {
                const long long k = length0 + s[(long long)t * B];
                if (k >= 0 && k < capacity) by_agent[k * N + a] = acc;
                acc = 0.0;
            }
        }
        carry[(long long)e * (N + 1) + a] = acc;
    } else {                                       // env e's total: N additions per step, agents ascending
        const int e = (int)(g - shares);
        double acc = carry[(long long)e * (N + 1) + N];
        const float *r = rew + (long long)e * N;
        const uint8_t *f = terminal + e;
        const int *s = slot + e;
        for (int t = 0; t < T; ++t) {
            const float *row = r + (long long)t * shares;
            for (int a = 0; a < N; ++a) acc += (double)row[a];
            if (f[(long long)t * B]) {
                const long long k = length0 + s[(long long)t * B];
                if (k >= 0 && k < capacity) {
                    total[k] = acc;
                    end_step[k] = step0 + t;
                    env[k] = e;
                }
                acc = 0.0;
            }
        }
        carry[(long long)e * (N + 1) + N] = acc;
    }
}

}  // namespace
