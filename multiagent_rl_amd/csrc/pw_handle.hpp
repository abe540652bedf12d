// pw_handle.hpp -- part of libpworld.so: the handle and the host-side helpers of the translation units that take one
// (pworld.hip, pworld_policy.hip, pworld_replay.hip).
#pragma once

#include <cstring>

#include "pw_host.hpp"
#include "pw_params.hpp"

struct pw_handle {
    pw_config cfg;
    KParams kp;
    pw_state_layout layout;
    bool bound;
    bool fast;      // pw_spread_fast_kernel applies
    FastConsts fc;
    bool tag_fast;  // pw_tag_stream_kernel applies
    TagParams tp;   // its constant part (pointers are filled per launch)
    float *comm;    // simple_reference planes inside the bound state block
    int32_t *goal;
    const char *last_kernel;  // name of the kernel the last pw_step / pw_rollout launched (pw_rollout_kernel)
    pw_dispatch disp;         // kernel selection: fixed by pw_create / pw_set_dispatch, never read from the environment at launch
    int actor_bf16x3;         // pw_set_actor_precision: 1 = the opt-in, NOT exact bf16x3 input projection of the one-launch rollouts
};

namespace {

// kernel parameter block of the communication scenarios (pw_kernels_reference.hpp) from a handle
RefParams ref_params(const pw_handle *h)
{
    const KParams &kp = h->kp;
    RefParams R;
    std::memset(&R, 0, sizeof(R));
    R.B = kp.B; R.L = kp.L; R.D = kp.D; R.max_episode_len = kp.max_episode_len; R.auto_reset = kp.auto_reset;
    R.force_discrete = kp.force_discrete; R.seed = kp.seed; R.env_id_base = kp.env_id_base;
    R.dt = kp.dt; R.damp = kp.damp; R.mass = kp.mass; R.sens = kp.agent_sens[0];
    R.pos_x = kp.pos_x; R.pos_y = kp.pos_y; R.vel_x = kp.vel_x; R.vel_y = kp.vel_y; R.lm_x = kp.lm_x; R.lm_y = kp.lm_y;
    R.comm = h->comm; R.goal = h->goal; R.ep_step = kp.ep_step; R.ep_count = kp.ep_count;
    return R;
}

// the simple_spread streaming kernels' block from a handle and a step's outputs; act, coll and p_prio stay with the caller
StreamParams stream_params(const pw_handle *h, const pw_step_io *io)
{
    const KParams &kp = h->kp;
    StreamParams A = {};
    A.B = kp.B; A.N = kp.N; A.L = kp.L; A.epw = kp.epw;
    A.max_episode_len = kp.max_episode_len; A.auto_reset = kp.auto_reset;
    A.seed = kp.seed; A.env_id_base = kp.env_id_base;
    A.dt = kp.dt; A.damp = kp.damp; A.contact_force = kp.contact_force; A.contact_margin = kp.contact_margin;
    A.mass = kp.mass;
    A.dist_min = h->fc.dist_min; A.coll_thr2 = h->fc.coll_thr2; A.near_thr2 = h->fc.near_thr2;
    A.sens = h->fc.sens; A.fscale = h->fc.fscale;
    A.pos_x = kp.pos_x; A.pos_y = kp.pos_y; A.vel_x = kp.vel_x; A.vel_y = kp.vel_y;
    A.lm_x = kp.lm_x; A.lm_y = kp.lm_y; A.ep_step = kp.ep_step; A.ep_count = kp.ep_count;
    A.obs = io->obs; A.final_obs = io->final_obs; A.rew = io->rew; A.rew_shared = io->rew_shared;
    A.done = io->done; A.terminal = io->terminal;
    return A;
}

// the simple_tag kernels' block: the handle's constant part + state planes and a step's outputs; act, coll, p_prio, obs_block stay with the caller
TagParams tag_params(const pw_handle *h, const pw_step_io *io)
{
    const KParams &kp = h->kp;
    TagParams A = h->tp;
    A.pos_x = kp.pos_x; A.pos_y = kp.pos_y; A.vel_x = kp.vel_x; A.vel_y = kp.vel_y;
    A.lm_x = kp.lm_x; A.lm_y = kp.lm_y; A.ep_step = kp.ep_step; A.ep_count = kp.ep_count;
    A.obs = io->obs; A.final_obs = io->final_obs; A.rew = io->rew; A.rew_shared = io->rew_shared;
    A.done = io->done; A.terminal = io->terminal;
    return A;
}

int check_ready(const pw_handle *h)
{
    if (!h) return fail(PW_EINVAL, "null handle");
    if (!h->bound) return fail(PW_ESTATE, "state block not bound: call pw_bind_state first");
    return PW_OK;
}

// The rollout sink of the single-head forms writes a single-head ROW ring, with the shared reward or (0.1.22) per agent.
int row_ring_only(const pw_replay_store *st, const char *who)
{
    if (st && st->act_heads > 1)
        return fail(PW_EINVAL, std::string(who) + ": a two-head ring is served by pw_replay_add, pw_replay_add_rollout, pw_replay_gather and "
                                                  "the simple_reference rollout sink only");
    if (st && st->state_rows)
        return fail(PW_EINVAL, std::string(who) + ": a STATE ring (pw_replay_store.state_rows) is filled by pw_replay_add_state_wire and read by "
                                                  "pw_replay_gather only -- observation rows cannot be turned back into the landmarks they were built from");
    return PW_OK;
}

// The tail / packed / wire entry points write the plain ring layout only: the blocks they read carry the shared reward.
int plain_ring_only(const pw_replay_store *st, const char *who)
{
    if (st && st->per_agent)
        return fail(PW_EINVAL, std::string(who) + ": a per-agent ring is served by pw_replay_add, pw_replay_add_rollout, pw_replay_gather, "
                                                  "pw_replay_sample and the pw_policy_rollout sink only (two-head / per-agent wire blocks are not served)");
    return row_ring_only(st, who);
}

// A state ring's own consistency (pw_replay_add_state_wire, pw_replay_gather, pw_replay_sample, the rollout sink).  Single-head; the
// reward planes may be per-agent (0.1.22: filled by the rollout sink; 0.1.23: and by pw_replay_add_state_wire_agents -- pw_replay_add_state_wire
// refuses that ring itself).
int state_ring_ok(const pw_replay_store *st, const char *who)
{
    if (st->act_heads > 1) return fail(PW_EINVAL, std::string(who) + ": a STATE ring is a single-head ring (two-head rings are row rings)");
    const int N = st->num_agents, L = st->num_landmarks, A = st->num_adversaries;
    if (!st->lm && L > 0) return fail(PW_EINVAL, std::string(who) + ": STATE ring without a landmark plane");
    if (N < 1 || L < 0 || A < 0 || A > N) return fail(PW_EINVAL, std::string(who) + ": bad STATE ring shape");
    const int D = st->scenario == PW_SIMPLE_SPREAD ? 4 + 2 * L : st->scenario == PW_SIMPLE_TAG ? 4 + 2 * L + 2 * (N - 1) + 2 * (N - A) : -1;
    if (D != st->obs_dim)
        return fail(PW_EINVAL, std::string(who) + ": STATE rings serve simple_spread (local observation, D = 4 + 2L) and simple_tag (D = 4 + 2L + 2(N - 1) + 2(N - A))");
    if ((reinterpret_cast<uintptr_t>(st->obs) | reinterpret_cast<uintptr_t>(st->next_obs)) & 15) return fail(PW_EINVAL, std::string(who) + ": STATE ring planes must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(st->lm) & 7) return fail(PW_EINVAL, std::string(who) + ": STATE ring landmark plane must be 8-byte aligned");
    return PW_OK;
}
}  // namespace
