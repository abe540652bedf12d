// pw_kernels_policy_generic.hpp -- part of libpworld.so (translation unit csrc/pworld_policy_generic.hip includes it).
// Policy-in-the-loop rollout for every simple_spread / simple_tag configuration pw_rollout_kernel serves (full observation, L > N,
// landmark contact, per-agent sizes / accelerations / speed clamps, a roster with one agent unlike its role): pw_policy_rollout_tag_kernel's
// structure (actor pass of the whole workgroup, then the last waves advance the environments) with pw_rollout_kernel's arithmetic,
// operation for operation, through the same pw_common.hpp device functions.
#pragma once

#include "pw_common.hpp"
#include "pw_kernels_actor16.hpp"
#include "pw_policy_shared.hpp"

namespace {

struct PolicyRolloutGenericArgs {
    ActorFusedArgs A;   // weights, B, N, D, E, heads, seed, step / step_dev (Philox step of the FIRST pass)
    KParams K;          // world constants, per-agent tables, state planes (K.epw unused: the layout function has this kernel's)
    float *obs, *final_obs, *rew, *rew_shared;   // the pw_step_io outputs, [T, ...]
    uint8_t *done, *terminal;
    int T;
    int32_t *act_out;   // [T,B,N] sampled action indices (or NULL)
    RolloutSink sink;   // optional direct sink (pw_policy_shared.hpp)
};

// The actor16 block, then the rollout's own regions.  Whole environments per environment wave: epw = min(E, 64 / N) of them, each
// wave with its own {pos, vel, lm, red} slice (the Smem of pw_rollout_kernel's one-wave workgroup).
struct PolicyGenericLds {
    Actor16Lds a16; float *s_obs; int32_t *s_act; float2 *s_pos, *s_vel, *s_lm; float *s_red; double *s_fs; int *s_fc; float *s_noise;
    unsigned char *red;   // alias, rollout_finish_stats' 8 KB over the start of the block
    int epw, env_waves; uint32_t bytes;
};
__host__ __device__ inline PolicyGenericLds policy_generic_lds(int S1, int D, int E, int N, int L, unsigned char *raw = nullptr)
{
    PolicyGenericLds o; o.a16 = actor16_lds(N, E * N, S1, raw);
    LdsCursor c = LdsCursor::after(raw, o.a16.bytes, o.a16.end);
    o.epw = E < kWave / N ? E : kWave / N; o.env_waves = (E + o.epw - 1) / o.epw;
    o.s_obs = c.take<float>(E * N * D, 16); o.s_act = c.take<int32_t>(E * N);   // [E * N][D] observation rows (16-byte row stores at D % 4 == 0), [E * N]
    o.s_pos = c.take<float2>(o.env_waves * kWave, 8); o.s_vel = c.take<float2>(o.env_waves * kWave, 8);   // [env waves][64] each
    o.s_lm = c.take<float2>(o.env_waves * o.epw * L, 8);   // [env waves][epw * L]
    o.s_red = c.take<float>(o.env_waves * o.epw * L);      // [env waves][epw * L] per-landmark minimum distance (L > N)
    o.s_fs = c.take<double>(16, 8); o.s_fc = c.take<int>(16);   // [16] each: finished-episode (sum, count) per environment
    o.s_noise = reinterpret_cast<float *>(c.take<float4>(actor16_noise_blocks(E * N, 5), 16));   // [E * N][2 blocks][4] Gumbel noise of the coming head
    o.red = raw; o.bytes = 4 * c.at; return o;
}

template <int SCEN, int OBS, int S1C, bool SINK>
__global__ void __launch_bounds__(512) pw_policy_rollout_generic_kernel(const PolicyRolloutGenericArgs P)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const ActorFusedArgs &A = P.A;
    const KParams &K = P.K;
    const int N = K.N, L = K.L, D = K.D;
    const PolicyGenericLds Y = policy_generic_lds(4 * S1C, D, A.E, N, L, smem_raw);
    const Actor16Lds &S = Y.a16;
    Actor16W W;  // the actor's weights: registers for the whole launch (pw_kernels_actor16.hpp)
    actor16_load<S1C>(A, S, W);

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long env0 = (long)blockIdx.x * A.E;
    const int envs_here = (int)((long)A.B - env0 < (long)A.E ? (long)A.B - env0 : (long)A.E);
    const int rows_here = envs_here * N;
    const long row_base = env0 * N;
    const size_t BN = (size_t)A.B * N;

    // the LAST waves are environment lanes (the actor pass deals its dense1 blocks and head tiles from wave 0 up): whole environments per wave
    const int epw = Y.epw;
    const int n_env_waves = (envs_here + epw - 1) / epw;
    const int ewi = wave - (8 - n_env_waves);
    const bool env_wave = ewi >= 0;
    Lane ln;   // hand-built: make_lane is pw_rollout_kernel's one-wave mapping
    {
        int e_loc = lane / N, a = lane - e_loc * N;
        int el = ewi * epw + e_loc;
        const bool live = env_wave && e_loc < epw && el < envs_here;
        if (!live) { e_loc = 0; a = 0; el = env_wave ? ewi * epw : 0; }  // idle lanes shadow the wave's first lane, store nothing
        ln.e_local = e_loc; ln.a = a; ln.base = e_loc * N;
        ln.env = (int)(env0 + el);
        ln.g = (size_t)ln.env * N + a;
        ln.valid = live;
    }
    const bool live = ln.valid;
    const int r_lane = (ln.env - (int)env0) * N + ln.a;   // row of the workgroup (env-major)
    const int ew = env_wave ? ewi : 0;
    float2 *s_pos = Y.s_pos + ew * kWave, *s_vel = Y.s_vel + ew * kWave, *s_lm = Y.s_lm + ew * epw * L;
    float *s_red = Y.s_red + ew * epw * L;

    float px = 0.f, py = 0.f, vx = 0.f, vy = 0.f;
    int ep_step = 0;
    uint32_t ep_count = 0;
    float my_size = 0.f, my_sens = 0.f, my_fscale = 1.f, my_maxspeed = -1.f;
    float ep_ret = 0.f;
    if (SINK) rollout_zero_episodes(Y.s_fs, Y.s_fc);
    if (env_wave) {
        if (live) {
            if (SINK && P.sink.episode_return && ln.a == 0) ep_ret = P.sink.episode_return[ln.env];
            px = K.pos_x[ln.g]; py = K.pos_y[ln.g];
            vx = K.vel_x[ln.g]; vy = K.vel_y[ln.g];
            ep_step = K.ep_step[ln.env];
            ep_count = K.ep_count[ln.env];
            my_size = K.agent_size[ln.a];
            my_sens = K.agent_sens[ln.a];
            my_fscale = K.agent_fscale[ln.a];
            my_maxspeed = K.agent_max_speed[ln.a];
            for (int l = ln.a; l < L; l += N)
                s_lm[ln.e_local * L + l] = make_float2(K.lm_x[(size_t)ln.env * L + l], K.lm_y[(size_t)ln.env * L + l]);
            s_pos[lane] = make_float2(px, py);
            if (SCEN == PW_SIMPLE_TAG) s_vel[lane] = make_float2(vx, vy);
        }
        wave_lds_sync();
        if (live) write_obs<SCEN, OBS>(K, ln, Y.s_obs + r_lane * D, px, py, vx, vy, s_pos, s_vel, s_lm);
    }
    const float k = K.contact_margin, cf = K.contact_force, dt = K.dt, damp = K.damp, mass = K.mass;
    const float near_margin = 88.5f * k;
    const uint64_t step0 = A.step_dev ? (uint64_t)*A.step_dev : A.step;
    // the Gumbel noise of step t + 1 is drawn by the waves without environment duty while the environment waves advance step t
    const int noise_thr = (8 - n_env_waves) * kWave;
    actor16_draw_noise(A, Y.s_noise, rows_here, row_base, step0, tid, 512);
    wg_lds_barrier();

    // The rest of an environment step once the agents are advanced, in two pieces:
    //   tail_compute  reward and masks on the new positions, the ordered shared reward, the terminal rule, episode bookkeeping
    //   tail_stores   every global store of the step
    // In a step that ends no episode of the wave both run inside the NEXT actor pass (before its dense1 blocks / before its head tiles:
    // actor16_forward's pre / mid windows); a wave with an episode ending runs both, final_obs and the reset before it publishes the rows.
    // StepTail (pw_policy_shared.hpp), inline: with the struct the step loops grow by 1 .. 2 instructions (<0,0,2,true> 6046 -> 6047)
    int ai = 0, tail_t = 0, tail_stage = 0;  // tail_stage: 0 nothing pending, 1 tail_compute pending, 2 tail_stores pending
    float t_rw = 0.f, t_acc = 0.f;
    bool t_term = false;
    auto tail_compute = [&]() {
        uint64_t mask = 0;
        const float rw = reward_and_mask<SCEN>(K, ln, px, py, my_size, s_pos, s_lm, s_red, mask);
        float acc = 0.0f;   // np.sum(rew_n), run.py:46, in agent order
        for (int i = 0; i < N; ++i) acc += __shfl(rw, ln.base + i, kWave);
        ep_step += 1;
        t_term = K.max_episode_len > 0 && ep_step >= K.max_episode_len;
        t_rw = rw;
        t_acc = acc;
        if (SINK && live && ln.a == 0 && P.sink.episode_return)
            episode_account(ep_ret, acc, t_term, Y.s_fs[ln.env - (int)env0], Y.s_fc[ln.env - (int)env0]);
    };
    auto tail_stores = [&](const int t, const bool with_obs) {  // with_obs: the obs output too (no reset in between: the same row)
        const size_t row = (size_t)t * BN + ln.g;
        if (live) {
            if (P.act_out) P.act_out[row] = ai;
            if (P.rew) P.rew[row] = t_rw;
            if (P.done) P.done[row] = 0;
            if (ln.a == 0) {
                if (P.rew_shared) P.rew_shared[(size_t)t * A.B + ln.env] = t_acc;
                if (P.terminal) P.terminal[(size_t)t * A.B + ln.env] = t_term ? 1 : 0;
            }
            // with_obs: next_obs and obs are both the row this lane published in LDS -- copied, not rebuilt
            // (copy_row2, inline at the three sites of this kernel: with the function 11 of 48 instantiations miss the codegen rule)
            const float2 *src = reinterpret_cast<const float2 *>(Y.s_obs + r_lane * D);
            if (SINK && P.sink.has_ring) {  // next_obs is the PRE-reset observation (run.py:52 vs :60)
                const size_t slot = ring_slot(P.sink.ring_start, t, A.B, (long)ln.env, P.sink.ring.capacity);
                float *dst = P.sink.ring.next_obs + (slot * N + ln.a) * D;
                if (with_obs) for (int c = 0; c < D / 2; ++c) reinterpret_cast<float2 *>(dst)[c] = src[c];
                else write_obs<SCEN, OBS>(K, ln, dst, px, py, vx, vy, s_pos, s_vel, s_lm);
                sink_reward(P.sink.ring, slot, N, ln.a, t_rw, t_acc);
            }
            if (with_obs && P.obs) {
                float2 *dst = reinterpret_cast<float2 *>(P.obs + row * D);
                for (int c = 0; c < D / 2; ++c) dst[c] = src[c];
            }
        }
    };
    auto pre_hook = [&]() { if (tail_stage == 1) { tail_compute(); tail_stage = 2; } };
    auto mid_hook = [&]() { if (tail_stage == 2) { tail_stores(tail_t, true); tail_stage = 0; } };

    for (int t = 0; t < P.T; ++t) {
        actor16_forward<S1C, false>(A, S, W, Y.s_obs, D, rows_here, envs_here, row_base, step0 + (uint64_t)t, nullptr, Y.s_act, pre_hook,
                                    mid_hook, Y.s_noise);  // a barrier at its end
        if (t + 1 < P.T && tid < noise_thr) actor16_draw_noise(A, Y.s_noise, rows_here, row_base, step0 + (uint64_t)(t + 1), tid, noise_thr);
        if (env_wave) {
            const size_t row = (size_t)t * BN + ln.g;  // flattened [t, env, agent]
            ai = Y.s_act[r_lane];
            if (SINK && P.sink.has_ring && live) {  // the observation the policy acted on (still in LDS) -> ring.obs
                const size_t slot = ring_slot(P.sink.ring_start, t, A.B, (long)ln.env, P.sink.ring.capacity);
                const float2 *src = reinterpret_cast<const float2 *>(Y.s_obs + r_lane * D);
                float2 *dst = reinterpret_cast<float2 *>(P.sink.ring.obs + (slot * N + ln.a) * D);
                for (int c = 0; c < D / 2; ++c) dst[c] = src[c];
                P.sink.ring.act[slot * N + ln.a] = (uint8_t)ai;
            }
            // ---- U2 _set_action + U4 apply_action_force
            if (live) {
                float ux = 0.0f + ((ai == 1 ? 1.0f : 0.0f) - (ai == 2 ? 1.0f : 0.0f));
                float uy = 0.0f + ((ai == 3 ? 1.0f : 0.0f) - (ai == 4 ? 1.0f : 0.0f));
                ux *= my_sens; uy *= my_sens;
                if (my_fscale != 1.0f) { ux = my_fscale * ux; uy = my_fscale * uy; }
                float fx = ux + 0.0f, fy = uy + 0.0f;
                // ---- U5 apply_environment_force: the near pass, then the marked partners in ascending order (agents, then landmarks)
                const float2 *pp = s_pos + ln.base;
                const float2 *lm = s_lm + ln.e_local * L;
                uint64_t near_a = 0, near_l = 0;
                for (int j = 0; j < N; ++j) {
                    const float2 q = pp[j];
                    const float dx = px - q.x, dy = py - q.y;
                    if (j != ln.a && !provably_far(dx * dx + dy * dy, my_size + K.agent_size[j], near_margin))
                        near_a |= 1ull << j;
                }
                if (K.landmark_collide) {
                    for (int l = 0; l < L; ++l) {
                        const float2 q = lm[l];
                        const float dx = px - q.x, dy = py - q.y;
                        if (!provably_far(dx * dx + dy * dy, my_size + K.landmark_size, near_margin)) near_l |= 1ull << l;
                    }
                }
                for (uint64_t m = near_a; m; m &= m - 1) {
                    const int j = __builtin_ctzll(m);
                    const float2 q = pp[j];
                    collision_force(px, py, q.x, q.y, my_size + K.agent_size[j], k, cf, fx, fy);
                }
                for (uint64_t m = near_l; m; m &= m - 1) {
                    const float2 q = lm[__builtin_ctzll(m)];
                    collision_force(px, py, q.x, q.y, my_size + K.landmark_size, k, cf, fx, fy);
                }
                // ---- U6 integrate_state
                vx = vx * damp; vy = vy * damp;
                vx = vx + (fx / mass) * dt;
                vy = vy + (fy / mass) * dt;
                if (my_maxspeed >= 0.0f) {
                    const float speed = sqrtf(vx * vx + vy * vy);
                    if (speed > my_maxspeed) {
                        vx = vx / speed * my_maxspeed;
                        vy = vy / speed * my_maxspeed;
                    }
                }
                px = px + vx * dt;
                py = py + vy * dt;
            }
            wave_lds_sync();  // every lane has read the old positions
            if (live) {
                s_pos[lane] = make_float2(px, py);
                if (SCEN == PW_SIMPLE_TAG) s_vel[lane] = make_float2(vx, vy);
            }
            wave_lds_sync();
            const bool ends = live && K.auto_reset && K.max_episode_len > 0 && ep_step + 1 >= K.max_episode_len;
            if (__any(ends)) {
                tail_compute();
                tail_stores(t, false);
                // ---- auto-reset (run.py:59-60): final_obs before reset_lane, then the post-reset row
                const bool do_reset = live && t_term && K.auto_reset;
                if (do_reset && P.final_obs)
                    write_obs<SCEN, OBS>(K, ln, P.final_obs + row * D, px, py, vx, vy, s_pos, s_vel, s_lm);
                wave_lds_sync();
                if (do_reset) {
                    ep_count += 1;
                    ep_step = 0;
                    reset_lane(K, ln, ep_count, SCEN, px, py, s_lm);
                    vx = 0.f; vy = 0.f;
                    s_pos[lane] = make_float2(px, py);
                    if (SCEN == PW_SIMPLE_TAG) s_vel[lane] = make_float2(0.f, 0.f);
                }
                wave_lds_sync();
                if (live) {
                    if (P.obs) write_obs<SCEN, OBS>(K, ln, P.obs + row * D, px, py, vx, vy, s_pos, s_vel, s_lm);
                    write_obs<SCEN, OBS>(K, ln, Y.s_obs + r_lane * D, px, py, vx, vy, s_pos, s_vel, s_lm);
                }
            } else {
                if (live) write_obs<SCEN, OBS>(K, ln, Y.s_obs + r_lane * D, px, py, vx, vy, s_pos, s_vel, s_lm);
                tail_stage = 1;
                tail_t = t;
            }
        }
        wg_lds_barrier();
    }
    if (tail_stage == 1) tail_compute();
    if (tail_stage != 0) tail_stores(tail_t, true);

    if (live) {
        K.pos_x[ln.g] = px; K.pos_y[ln.g] = py;
        K.vel_x[ln.g] = vx; K.vel_y[ln.g] = vy;
        for (int l = ln.a; l < L; l += N) {
            const float2 q = s_lm[ln.e_local * L + l];
            K.lm_x[(size_t)ln.env * L + l] = q.x;
            K.lm_y[(size_t)ln.env * L + l] = q.y;
        }
        if (ln.a == 0) {
            K.ep_step[ln.env] = ep_step;
            K.ep_count[ln.env] = ep_count;
            if (SINK && P.sink.episode_return) P.sink.episode_return[ln.env] = ep_ret;
        }
    }
    if (SINK) rollout_finish_episodes(P.sink, envs_here, Y.s_fs, Y.s_fc, Y.red);
}

}  // namespace
