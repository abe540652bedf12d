// pw_kernels_policy_ref.hpp -- part of libpworld.so (translation unit csrc/pworld_policy.hip).
// Policy-in-the-loop rollout as ONE launch for simple_reference, the MultiDiscrete scenario of the reference's sweep
// (main.py:24, :52-54: a two-head actor [5 movement | 10 communication logits]; experiments/run.py:39-41 concatenates
// the heads' one-hots into the env action).
#pragma once

#include "pw_kernels_reference.hpp"
#include "pw_kernels_actor16.hpp"
#include "pw_policy_shared.hpp"

namespace {

// ------------------------------------------------------------------------------------------
// T x (two-head actor forward + one Gumbel-argmax per head + environment step + auto-reset) per workgroup of 16
// environments (32 observation rows: N = 2), observations / sampled (movement, symbol) pairs / world state resident on the
// CU between steps -- the simple_reference counterpart of pw_policy_rollout_kernel.  The actor pass is actor16_forward
// (pw_kernels_actor16.hpp: the arithmetic and Philox keying of pw_actor_fused with n_out0 = 5, n_out1 = 10); the environment step is
// pw_reference_rollout_kernel's arithmetic on the workgroup's first wave (lane = (env, agent), the partner is lane ^ 1,
// every exchange a shuffle), so the results equal the loop "act = pw_actor_fused(obs); pw_step(act)" bit for bit.
// Outputs as pw_rollout's; act_out [T,B,N,2] int32 = (movement index, symbol index).
// ------------------------------------------------------------------------------------------
struct PolicyRolloutRefArgs {
    ActorFusedArgs A;   // weights, B, N = 2, D = 21, E, heads (5, dim_c), seed, step / step_dev (Philox step of the FIRST pass)
    RefParams V;        // world constants and state planes
    int T;
    int32_t *act_out;   // [T,B,N,2] (or NULL)
    float *obs, *final_obs, *rew, *rew_shared;
    uint8_t *done, *terminal;
    RolloutSink sink;   // optional direct sink (pw_policy_shared.hpp): the TWO-HEAD replay ring (act [cap,N,2] u8)
};

// The actor16 block (N = 2, 16 environments), then the rollout's own regions
struct PolicyRefLds {
    Actor16Lds a16; float *s_obs2, *s_noise; int32_t *s_act; double *s_fs; int *s_fc;
    unsigned char *red; uint32_t bytes;   // red: alias, rollout_finish_stats' 8 KB over the start of the block
};
__host__ __device__ inline PolicyRefLds policy_ref_lds(int S1, int D, int E, unsigned char *raw = nullptr)
{
    PolicyRefLds o; o.a16 = actor16_lds(2, E * 2, S1, raw);
    LdsCursor c = LdsCursor::after(raw, o.a16.bytes, o.a16.end);
    // observation rows, TWO buffers of [96][D]: the policy reads buffer `cur`, the environment lanes publish the next rows into the other
    // one -- so that, with a ring sink, the IDLE waves can copy the rows the policy acted on into ring.obs during the environment step
    o.s_obs2 = c.take<float>(2 * kFusedRows * D); o.s_act = c.take<int32_t>(2 * kFusedRows);   // s_act: [96][2] (movement, symbol)
    o.s_fs = c.take<double>(16); o.s_fc = c.take<int>(16);   // [16] each: finished-episode sums / counts (SINK)
    o.s_noise = reinterpret_cast<float *>(c.take<float4>(actor16_noise_blocks(32, 5 + kDimC), 16));   // [32][4 blocks][4] Gumbel noise of the coming heads (drawn a step ahead)
    o.red = raw; o.bytes = 4 * (c.at - c.pad) + 16; return o;   // trailing slack: the launch has always reserved 16 bytes for the noise's pad
}

#ifdef PW_STAMPS
__device__ unsigned long long g_pw_ref_stamps[30];
#endif
template <int S1C, bool SINK = false>
__global__ void __launch_bounds__(512) pw_policy_rollout_ref_kernel(const PolicyRolloutRefArgs P)
{
    constexpr int DC = kDimC, N = 2;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const ActorFusedArgs &A = P.A;
    const RefParams &V = P.V;
    const int D = A.D;
    const PolicyRefLds Y = policy_ref_lds(4 * S1C, D, A.E, smem_raw);
    const Actor16Lds &S = Y.a16;
    Actor16W W;  // the actor's weights: registers for the whole launch (pw_kernels_actor16.hpp)
    actor16_load<S1C>(A, S, W);
    Actor16D1<S1C> T1;  // dense1 as 16 x 16 tiles: with N = 2 the 32 x 32 form has two blocks for eight waves
    actor16_load_d1<S1C>(A, T1);

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long env0 = (long)blockIdx.x * A.E;
    const int envs_here = (int)((long)A.B - env0 < (long)A.E ? (long)A.B - env0 : (long)A.E);
    const int rows_here = envs_here * N;
    const long row_base = env0 * N;
    const size_t BN = (size_t)A.B * N;

    // ---- environment lanes (one wave, the partner is lane ^ 1: its own mapping, not env_waves' split): the LAST wave, lane = el * 2 + a
    // (E <= 16 envs: 32 lanes) -- the tail of a step (reward, stores) then runs
    // beside the next actor pass's dense1 blocks and head tiles, which sit on waves 0 and 1 (actor16_forward's pre / mid windows)
    const bool env_wave = wave == 7;
    int el = lane >> 1;
    const int a = lane & 1;
    const bool live = env_wave && el < envs_here;
    if (!live) el = 0;                  // idle lanes shadow env 0 of the workgroup (same agent parity: shuffles stay paired)
    const int r = el * N + a;
    const int env = (int)(env0 + el);
    const size_t g = (size_t)env * N + a;
    RefLane<DC> s;
    int ep_step = 0;
    uint32_t ep_count = 0;
    float ep_ret = 0.f;
    double fin_sum = 0.0;
    int fin_cnt = 0;
    size_t slot = 0;
    if (env_wave) {
        if (SINK && P.sink.episode_return && live && a == 0) ep_ret = P.sink.episode_return[env];
        ref_load<DC>(V, env, a, s);
        ep_step = V.ep_step[env];
        ep_count = V.ep_count[env];
        float co[DC];
#pragma unroll
        for (int q = 0; q < DC; ++q) co[q] = __shfl_xor(s.c[q], 1, kWave);
        if (live) ref_write_obs<DC, false>(V, s, co, a, Y.s_obs2 + r * D);
    }
    const uint64_t step0 = A.step_dev ? (uint64_t)*A.step_dev : A.step;
    actor16_draw_noise(A, Y.s_noise, rows_here, row_base, step0, tid, 512);
    wg_lds_barrier();

    // the rest of a step once the agents are advanced and the next observation rows published: rewards + episode step count
    // (tail_compute), every global store (tail_stores); a wave with an episode ending in this step does everything at once
    int ai = 0, ci = 0;
    StepTail tail;
    float co[DC];  // the other agent's symbol (this step's)
    auto tail_compute = [&]() {
        const float ox = __shfl_xor(s.px, 1, kWave), oy = __shfl_xor(s.py, 1, kWave);
        float glx, gly;
        ref_goal_landmark<DC>(s, s.goal, glx, gly);
        const float dx = ox - glx, dy = oy - gly;
        const float rw = -(dx * dx + dy * dy);
        const float r_other = __shfl_xor(rw, 1, kWave);
        tail.rw = rw;
        tail.acc = (0.0f + (a == 0 ? rw : r_other)) + (a == 0 ? r_other : rw);  // agent order
        ep_step += 1;
        tail.term = V.max_episode_len > 0 && ep_step >= V.max_episode_len;
        // into registers, published after the loop: into LDS (rollout_zero_episodes / rollout_finish_episodes, as tag, generic and 3j) the
        // sink instantiation goes from 179 to 187 SGPR spills and its step loop from 2514 to 2536 instructions
        if (SINK && live && a == 0 && P.sink.episode_return) episode_account(ep_ret, tail.acc, tail.term, fin_sum, fin_cnt);
    };
    auto tail_stores = [&](const int t, const bool with_obs) {
        const size_t row = (size_t)t * BN + g;
        if (live) {
            if (P.act_out) { P.act_out[2 * row] = ai; P.act_out[2 * row + 1] = ci; }
            if (P.rew) P.rew[row] = tail.rw;
            if (P.done) P.done[row] = 0;
            if (a == 0) {
                if (P.rew_shared) P.rew_shared[(size_t)t * A.B + env] = tail.acc;
                if (P.terminal) P.terminal[(size_t)t * A.B + env] = tail.term ? 1 : 0;
            }
            if (with_obs && P.obs) ref_write_obs<DC, false>(V, s, co, a, P.obs + row * D);
            if (SINK && P.sink.has_ring) {  // next_obs is the PRE-reset observation (run.py:52 vs :60)
                ref_write_obs<DC, false>(V, s, co, a, P.sink.ring.next_obs + (slot * N + a) * D);
                sink_reward(P.sink.ring, slot, N, a, tail.rw, tail.acc);
            }
        }
    };
    auto pre_hook = [&]() { tail.pre(tail_compute); };
    auto mid_hook = [&]() { tail.mid(tail_stores); };

#ifdef PW_STAMPS
    unsigned long long rs[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, r0_ = 0, r1_ = 0;
    PW_R2_START;
#define PW_REF_STAMP_ARGS , rs, &r0_
#else
#define PW_REF_STAMP_ARGS
#endif
    for (int t = 0; t < P.T; ++t) {
        float *s_obs = Y.s_obs2 + (t & 1) * (kFusedRows * D);          // what the policy acts on in this step
        float *s_next = Y.s_obs2 + ((t + 1) & 1) * (kFusedRows * D);   // where the environment lanes publish the next rows
        // ---- policy: observation rows (LDS) -> one sampled index per head and row (LDS)
        actor16_forward<S1C, false>(A, S, W, s_obs, D, rows_here, envs_here, row_base, step0 + (uint64_t)t, nullptr, Y.s_act, pre_hook,
                                    mid_hook, Y.s_noise, &T1 PW_REF_STAMP_ARGS);  // a barrier at its end
        // the noise of the NEXT step's heads: by the seven waves that wait for the environment wave
        if (t + 1 < P.T && !env_wave) actor16_draw_noise(A, Y.s_noise, rows_here, row_base, step0 + (uint64_t)(t + 1), tid, 7 * kWave);
        if (SINK && P.sink.has_ring && !env_wave) {
            // the observations the policy acted on -> ring.obs, by the seven waves that would otherwise wait for the environment wave
            for (int idx = tid; idx < rows_here * D; idx += 448) {
                const int rr = idx / D, c = idx - rr * D;
                const size_t sl = ring_slot(P.sink.ring_start, t, A.B, env0 + (rr >> 1), P.sink.ring.capacity);
                P.sink.ring.obs[(sl * N + (rr & 1)) * D + c] = s_obs[idx];
            }
        }
        PW_R2_STAMP(7);
        // ---- environment step (pw_reference_rollout_kernel's arithmetic, index actions)
        if (env_wave) {
            const size_t row = (size_t)t * BN + g;
            ai = Y.s_act[2 * r]; ci = Y.s_act[2 * r + 1];
            if (SINK && P.sink.has_ring) {  // the pair the policy sampled -> ring.act (the observation rows: the idle waves, above)
                slot = ring_slot(P.sink.ring_start, t, A.B, (long)env, P.sink.ring.capacity);
                if (live) {
                    P.sink.ring.act[(slot * N + a) * 2] = (uint8_t)ai;
                    P.sink.ring.act[(slot * N + a) * 2 + 1] = (uint8_t)ci;
                }
            }
            const float a1 = ai == 1, a2 = ai == 2, a3 = ai == 3, a4 = ai == 4;
            float cn[DC];
#pragma unroll
            for (int q = 0; q < DC; ++q) cn[q] = q == ci ? 1.0f : 0.0f;
            {
                float ux = 0.0f + (a1 - a2), uy = 0.0f + (a3 - a4);
                ux *= V.sens; uy *= V.sens;
                const float fx = ux + 0.0f, fy = uy + 0.0f;
                s.vx = s.vx * V.damp; s.vy = s.vy * V.damp;
                s.vx = s.vx + (fx / V.mass) * V.dt;
                s.vy = s.vy + (fy / V.mass) * V.dt;
                s.px = s.px + s.vx * V.dt;
                s.py = s.py + s.vy * V.dt;
            }
#pragma unroll
            for (int q = 0; q < DC; ++q) s.c[q] = cn[q] + 0.0f;
#pragma unroll
            for (int q = 0; q < DC; ++q) co[q] = __shfl_xor(s.c[q], 1, kWave);
            const bool ends = V.auto_reset && V.max_episode_len > 0 && ep_step + 1 >= V.max_episode_len;
            if (__any(ends)) {
                tail_compute();
                tail_stores(t, false);
                if (tail.term && V.auto_reset) {
                    if (live && P.final_obs) ref_write_obs<DC, false>(V, s, co, a, P.final_obs + row * D);
                    ep_count += 1;
                    ep_step = 0;
                    ref_reset<DC, false>(V, V.env_id_base + (uint64_t)env, ep_count, a, s);
#pragma unroll
                    for (int q = 0; q < DC; ++q) co[q] = 0.f;  // the other agent reset too
                }
                if (live) {
                    if (P.obs) ref_write_obs<DC, false>(V, s, co, a, P.obs + row * D);
                    ref_write_obs<DC, false>(V, s, co, a, s_next + r * D);
                }
            } else {
                if (live) ref_write_obs<DC, false>(V, s, co, a, s_next + r * D);
                tail.defer(t);
            }
        }
        PW_R2_STAMP(8);
        wg_lds_barrier();
        PW_R2_STAMP(9);
    }
#ifdef PW_STAMPS
    if (blockIdx.x == 0 && lane == 0 && (wave == 0 || wave == 7 || wave == 3))
        for (int i_ = 0; i_ < 10; ++i_) g_pw_ref_stamps[(wave == 0 ? 0 : wave == 7 ? 1 : 2) * 10 + i_] = rs[i_];
#endif
    tail.flush(tail_compute, tail_stores);
    if (live) {
        ref_store<DC>(V, env, a, s);
        if (a == 0) {
            V.ep_step[env] = ep_step; V.ep_count[env] = ep_count;
            if (SINK && P.sink.episode_return) P.sink.episode_return[env] = ep_ret;
        }
    }
    if (SINK && P.sink.episode_return) {  // finished-episode statistics: per-workgroup partials, the last workgroup adds them up in order
        wg_lds_barrier();
        if (live && a == 0) { Y.s_fs[el] = fin_sum; Y.s_fc[el] = fin_cnt; }
        wg_lds_barrier();
        rollout_finish_stats(envs_here, Y.s_fs, Y.s_fc, P.sink.scratch, P.sink.finished_sum, P.sink.finished_count, Y.red);
    }
}

}  // namespace
