// pw_policy_shared.hpp -- part of libpworld.so (translation units csrc/pworld_policy.hip and csrc/pworld_policy_generic.hip include it).
// Helpers shared by the five one-launch policy rollout kernels (pw_kernels_policy3.hpp, pw_kernels_policy3j.hpp, pw_kernels_policy_tag.hpp,
// pw_kernels_policy_ref.hpp, pw_kernels_policy_generic.hpp): the LDS observation row writer and row copy, the environment-wave split,
// opaque(), the ordered shuffles, the rollout sink and its ring helpers, the deferred step tail, the episode accounting and the stamp /
// debug macros of the PW_STAMPS probe builds.  profiles/rollout_tail_codegen.txt: what the compiler made of each, and what stayed inline.
#pragma once

#include "pw_common.hpp"
#include "pw_lstm_math.hpp"

namespace {

// observation row into LDS with 8-byte stores (the LDS rows are only 8-byte aligned: stride D + 2)
template <int LT>
__device__ __forceinline__ void lds_write_obs_row(float *o, const int L, const float2 *lm, float px, float py, float vx,
                                                  float vy)
{
    float2 *o2 = reinterpret_cast<float2 *>(o);
    o2[0] = make_float2(vx, vy);
    o2[1] = make_float2(px, py);
    if (LT > 0) {
#pragma unroll
        for (int l = 0; l < LT; ++l) {
            const float2 q = lm[l];
            o2[2 + l] = make_float2(q.x - px, q.y - py);
        }
    } else {  // runtime L: four landmark reads in flight per round (one LDS round trip per landmark otherwise: ~1.2 k cycles at L = 12)
        int l = 0;
        for (; l + 4 <= L; l += 4) {
            const float2 q0 = lm[l], q1 = lm[l + 1], q2 = lm[l + 2], q3 = lm[l + 3];
            o2[2 + l] = make_float2(q0.x - px, q0.y - py);
            o2[3 + l] = make_float2(q1.x - px, q1.y - py);
            o2[4 + l] = make_float2(q2.x - px, q2.y - py);
            o2[5 + l] = make_float2(q3.x - px, q3.y - py);
        }
        for (; l < L; ++l) {
            const float2 q = lm[l];
            o2[2 + l] = make_float2(q.x - px, q.y - py);
        }
    }
}

// Environment lanes of a workgroup of E environments with N agents each (lane = (environment, agent), whole environments per wave):
// as few waves as hold E, the environments spread evenly over them -> epw environments per wave, and the waves that the
// envs_here <= E environments of THIS workgroup occupy
struct EnvWaves {
    int epw, n_waves;
};
__device__ __forceinline__ EnvWaves env_waves(const int E, const int N, const int envs_here)
{
    const int epw_max = E < kWave / N ? E : kWave / N;
    const int waves_full = (E + epw_max - 1) / epw_max;
    EnvWaves w;
    w.epw = (E + waves_full - 1) / waves_full;
    w.n_waves = (envs_here + w.epw - 1) / w.epw;
    return w;
}

// LDS row -> global row, n2 = D / 2 8-byte words (the LDS rows are only 8-byte aligned)
__device__ __forceinline__ void copy_row2(float *dst, const float *src, const int n2)
{
    for (int c = 0; c < n2; ++c) reinterpret_cast<float2 *>(dst)[c] = reinterpret_cast<const float2 *>(src)[c];
}

// A lane's launch-invariant global index passes through this empty asm wherever it feeds an output address: otherwise every
// `pointer + g` of a step's stores is computed once per launch and kept in a register pair for the whole kernel -- what pushed the
// widest rollout instantiations over the 256-register cap and into scratch memory; a few address additions per step are cheaper
__device__ __forceinline__ uint32_t opaque(const uint32_t v)
{
    uint32_t x = v;
    asm volatile("" : "+v"(x));
    return x;
}

#ifdef PW_STAMPS
__device__ int g_pw_debug;  // probe builds only: bit 0 skips the MFMAs (tiles still announced), bit 1 the recurrences
#define PW_DBG(bit) (g_pw_debug & (bit))
#else
#define PW_DBG(bit) 0
#endif

#ifdef PW_STAMPS
#define PW_R2_DECL unsigned long long rs[8] = {0, 0, 0, 0, 0, 0, 0, 0}, r0_ = 0, r1_ = 0
#define PW_R2_START asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(r0_)::"memory")
#define PW_R2_STAMP(i) do { asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(r1_)::"memory"); rs[i] += r1_ - r0_; r0_ = r1_; } while (0)
#define PW_R2_FLUSH(base) do { if (blockIdx.x == 0 && lane == 0) for (int i_ = 0; i_ < 8; ++i_) g_pw_stamps[(base) + i_] = rs[i_]; } while (0)
#else
#define PW_R2_DECL
#define PW_R2_START
#define PW_R2_STAMP(i)
#define PW_R2_FLUSH(base)
#endif

// Ordered per-env reductions by wave shuffle for a runtime agent count: acc (+/-)= shfl(v, base + i) for i = 0 .. n - 1 IN THAT ORDER
// (the upstream summation order: the bits depend on it), with four shuffles in flight per round -- issued one at a time, each
// ds_bpermute's ~120-cycle round trip is exposed: 36 of them per step at N = 12, 72 at N = 24, on the environment waves' critical path.
__device__ __forceinline__ float shfl_sub_ordered(float acc, const float v, const int base, const int n)
{
    int i = 0;
    for (; i + 4 <= n; i += 4) {
        const float a0 = __shfl(v, base + i, kWave), a1 = __shfl(v, base + i + 1, kWave);
        const float a2 = __shfl(v, base + i + 2, kWave), a3 = __shfl(v, base + i + 3, kWave);
        acc -= a0; acc -= a1; acc -= a2; acc -= a3;
    }
    for (; i < n; ++i) acc -= __shfl(v, base + i, kWave);
    return acc;
}
__device__ __forceinline__ float shfl_add_ordered(float acc, const float v, const int base, const int n)
{
    int i = 0;
    for (; i + 4 <= n; i += 4) {
        const float a0 = __shfl(v, base + i, kWave), a1 = __shfl(v, base + i + 1, kWave);
        const float a2 = __shfl(v, base + i + 2, kWave), a3 = __shfl(v, base + i + 3, kWave);
        acc += a0; acc += a1; acc += a2; acc += a3;
    }
    for (; i < n; ++i) acc += __shfl(v, base + i, kWave);
    return acc;
}

// Optional direct sink of a one-launch rollout (one member of every kernel's argument block; zeroed = no sink): the transitions go
// straight into the replay ring (slot (ring_start + t*B + env) % capacity, the order of T pw_replay_add calls; simple_reference: the
// TWO-HEAD ring, act [cap,N,2] u8) and the episode returns are kept here, so no second launch has to re-read the step outputs (which then
// may all be NULL)
struct RolloutSink {
    pw_replay_store ring;
    int has_ring;
    int64_t ring_start;
    float *episode_return;          // [B] running return per env (or NULL)
    double *finished_sum;
    int64_t *finished_count;
    unsigned long long *scratch;    // [1 + 2 * gridDim.x] words (ticket, partial sums, partial counts: rollout_finish_stats), zeroed once
};
// Ring sink of the one-launch rollouts into a STATE ring (pw_replay_store.state_rows: the planes hold {vx, vy, px, py} per agent and the episode's
// landmarks per transition; pw_replay_gather rebuilds the rows): the pre-step state + this lane's landmarks, and the post-step (pre-reset) state.
__device__ __forceinline__ void sink_state_obs(const pw_replay_store &ring, const size_t slot, const int N, const int a, const int L,
                                               const float2 *lmv, const float px, const float py, const float vx, const float vy)
{
    reinterpret_cast<float4 *>(ring.obs)[slot * N + a] = make_float4(vx, vy, px, py);
    for (int l = a; l < L; l += N) reinterpret_cast<float2 *>(ring.lm)[slot * L + l] = lmv[l];
}
__device__ __forceinline__ void sink_state_next(const pw_replay_store &ring, const size_t slot, const int N, const int a, const float px,
                                                const float py, const float vx, const float vy)
{
    reinterpret_cast<float4 *>(ring.next_obs)[slot * N + a] = make_float4(vx, vy, px, py);
}

// Reward and done flag of transition `slot`, by every live lane of the env: the shared ring takes the ordered sum `acc` from agent 0's
// lane; a per-agent ring (pw_replay_store.per_agent: planes [cap,N], the BiCNet tuple) takes the lane's own reward `rw` -- the value the
// launch writes to rew[t, env, a].  done is 0: these scenarios have no done callback.  The ring's kind is wave-uniform (a kernel argument).
__device__ __forceinline__ void sink_reward(const pw_replay_store &ring, const size_t slot, const int N, const int a, const float rw,
                                            const float acc)
{
    const bool pa = ring.per_agent != 0;
    if (pa || a == 0) {   // one pair of stores for both rings: the ring's kind selects the index and the value
        const size_t i = pa ? slot * N + a : slot;
        ring.rew[i] = pa ? rw : acc;
        ring.done[i] = 0.0f;
    }
}

// Ring slot of transition (t, env) of a chunk that starts at ring_start: (ring_start + t * B + env) mod capacity WITHOUT the 64-bit
// division (~150 instructions on the environment waves' critical path, every step): the host guarantees 0 <= ring_start < capacity and
// T * B <= capacity, so the sum is below 2 * capacity and one conditional subtraction is the modulo.
__device__ __forceinline__ size_t ring_slot(const int64_t ring_start, const int t, const int B, const long env, const int64_t capacity)
{
    const int64_t x = ring_start + (int64_t)t * B + env;
    return (size_t)(x >= capacity ? x - capacity : x);
}

// The rest of an environment step once the agents are advanced and the next observation rows published, in two pieces that the
// environment waves run inside the NEXT actor pass (actor16_forward's pre / mid windows):
//   compute()            partner pass / rewards / episode bookkeeping of step t -> rw, acc, term
//   stores(t, with_obs)  every global store of the step
// defer(t) leaves both pending; pre() runs the first, mid() the second, flush() after the step loop whatever is left.  A wave with an
// episode ending in the step runs both at once, with_obs = false, and defers nothing.
struct StepTail {
    int stage = 0, t = 0;   // stage: 0 nothing pending, 1 compute pending, 2 stores pending
    float rw = 0.f, acc = 0.f;
    bool term = false;
    __device__ __forceinline__ void defer(const int t_) { stage = 1; t = t_; }
    template <class C> __device__ __forceinline__ void pre(C &&compute) { if (stage == 1) { compute(); stage = 2; } }
    template <class S> __device__ __forceinline__ void mid(S &&stores) { if (stage == 2) { stores(t, true); stage = 0; } }
    template <class C, class S> __device__ __forceinline__ void flush(C &&compute, S &&stores)
    {
        if (stage == 1) compute();
        if (stage != 0) stores(t, true);
    }
};

// Finished-episode statistics of a rollout launch (run.py:55-65 bookkeeping summed over all envs): every workgroup leaves its
// partial (sum, count) in `scratch` (word 0: the ticket; then [gridDim.x] doubles, [gridDim.x] counts); the workgroup that takes the last
// ticket adds the partials up -- with ALL its threads: 512 partials per round through LDS and a fixed binary tree (deterministic:
// the pairing depends on gridDim.x alone) -- and clears the ticket.  The ticket's place must not depend on the launch's grid: one scratch
// serves every form a handle may launch (pw_dispatch.policy_form, bf16x3, two handles of equal B behind one actor), and behind a grid
// of another size lie the previous launch's partials, not zeros.  (Until 0.1.13 the ticket sat at word 2 * gridDim.x: a launch with fewer
// workgroups than its predecessor found a partial sum there, nobody drew the last ticket and the launch's episodes went uncounted.)  (Until round 4 one thread walked the partials one global load after the other: ~40 us at
// the end of every launch with 256 workgroups -- 3 % of a 100-step C2 chunk.)  Call with the per-env partials in s_fs / s_fc
// (LDS, complete: a barrier has passed); `red` = 8 KB of LDS that nothing else uses any more (the start of the block).
__device__ __forceinline__ void rollout_finish_stats(const int envs_here, double *s_fs, int *s_fc, unsigned long long *scratch,
                                                     double *finished_sum, int64_t *finished_count, unsigned char *red)
{
    const int tid = threadIdx.x;
    unsigned long long *ticket = scratch;
    double *part_sum = reinterpret_cast<double *>(scratch + 1);
    long long *part_cnt = reinterpret_cast<long long *>(scratch + 1 + gridDim.x);
    if (tid == 0) {
        double ws = 0.0;
        long long wc = 0;
        for (int i = 0; i < envs_here; ++i) { ws += s_fs[i]; wc += s_fc[i]; }
        part_sum[blockIdx.x] = ws;
        part_cnt[blockIdx.x] = wc;
        __threadfence();
        s_fc[0] = atomicAdd(ticket, 1ull) == (unsigned long long)gridDim.x - 1 ? 1 : 0;  // the per-env partials are consumed: reuse a slot
    }
    wg_lds_barrier();
    if (!s_fc[0]) return;   // workgroup-uniform
    __threadfence();
    double *red_s = reinterpret_cast<double *>(red);             // [512]
    long long *red_c = reinterpret_cast<long long *>(red) + 512;  // [512]
    double ssum = 0.0;
    long long scnt = 0;
    for (unsigned base = 0; base < gridDim.x; base += 512) {
        const unsigned i = base + (unsigned)tid;
        red_s[tid] = i < gridDim.x ? __builtin_nontemporal_load(part_sum + i) : 0.0;
        red_c[tid] = i < gridDim.x ? __builtin_nontemporal_load(part_cnt + i) : 0ll;
        wg_lds_barrier();
        for (int stride = 256; stride >= 1; stride >>= 1) {
            if (tid < stride) { red_s[tid] += red_s[tid + stride]; red_c[tid] += red_c[tid + stride]; }
            wg_lds_barrier();
        }
        if (tid == 0) { ssum += red_s[0]; scnt += red_c[0]; }
        wg_lds_barrier();
    }
    if (tid == 0) {
        *finished_sum += ssum;
        *finished_count += scnt;
        *ticket = 0;
    }
}

// Episode-return accounting of one env and step (run.py:55-65), by the env's agent-0 lane: acc = the step's shared reward; a finished
// episode's return goes to the env's (sum, count) pair and the running return starts over.  The pair lives in LDS (tag, generic, 3j:
// touched once per episode) or in registers that are published after the step loop (form 3, simple_reference).
__device__ __forceinline__ void episode_account(float &ep_ret, const float acc, const bool term, double &fs, int &fc)
{
    const float rsum = ep_ret + acc;
    if (term) { fs += (double)rsum; fc += 1; ep_ret = 0.0f; }
    else ep_ret = rsum;
}
// The per-env (sum, count) pairs of this launch start at zero (a workgroup barrier before the first episode_account)
__device__ __forceinline__ void rollout_zero_episodes(double *s_fs, int *s_fc)
{
    if (threadIdx.x < 16) { s_fs[threadIdx.x] = 0.0; s_fc[threadIdx.x] = 0; }
}
// ... and after the last step every workgroup hands them to rollout_finish_stats.  Workgroup-uniform; call with SINK only.
__device__ __forceinline__ void rollout_finish_episodes(const RolloutSink &K, const int envs_here, double *s_fs, int *s_fc,
                                                        unsigned char *red)
{
    if (!K.episode_return) return;
    wg_lds_barrier();
    rollout_finish_stats(envs_here, s_fs, s_fc, K.scratch, K.finished_sum, K.finished_count, red);
}

}  // namespace
