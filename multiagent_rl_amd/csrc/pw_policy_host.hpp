// pw_policy_host.hpp -- part of libpworld.so: the host-side helpers the two policy translation units share (csrc/pworld_policy.hip,
// csrc/pworld_policy_generic.hip): the actor's argument block and the checks / hand-over of a rollout sink.  No device code.
#pragma once

#include <cstring>

#include "pw_handle.hpp"
#include "pw_kernels_policy.hpp"

namespace {

// The part of ActorFusedArgs every launch form fills the same way: weights, sizes, heads, Philox seed / step and the
// environments per 96-row workgroup (the 16x16x4-core kernels override E).  X, H, logits, act and bf16x3 stay with the caller.
ActorFusedArgs actor_args(const float *frag, const float *b1, const float *b_ih, const float *w_hh_fw, const float *w_hh_bw,
                          const float *w2, const float *b2, int B, int N, int D, int relu_out, int n_out0, int n_out1,
                          uint64_t seed, uint64_t step, const int64_t *step_dev)
{
    ActorFusedArgs a = {};
    a.frag = frag; a.b1 = b1; a.bih = b_ih; a.whh_f = w_hh_fw; a.whh_r = w_hh_bw; a.w2 = w2; a.b2 = b2;
    a.B = B; a.N = N; a.D = D; a.relu_out = relu_out; a.n_out0 = n_out0; a.n_out1 = n_out1;
    a.E = 96 / N < 16 ? 96 / N : 16;
    a.seed = seed; a.step = step; a.step_dev = step_dev;
    return a;
}

// A sink that takes something off the launch -- the ring, the episode bookkeeping or both: only then may step outputs be left out
// (a launch that writes nothing at all is refused).  FusedActor.rollout(out=False, stats=...) is the statistics-only caller.
bool sink_takes(const pw_rollout_sink *sink) { return sink && (sink->ring || sink->episode_return); }

// A rollout sink's ring has the rollout's row shape and room for the chunk of `rows` transitions from a valid cursor, and its
// bookkeeping pointers come together.  The planes are the caller's: rew / done hold `capacity` floats, capacity * N on a per-agent ring
// (pw_replay_store.per_agent), and every slot the launch writes is below capacity.
int sink_fits(const pw_rollout_sink *sink, int N, int D, int64_t rows)
{
    const pw_replay_store *ring = sink->ring;
    if (ring && (ring->num_agents != N || ring->obs_dim != D || ring->capacity < 1 || sink->ring_start < 0 ||
                 sink->ring_start >= ring->capacity || rows > ring->capacity))
        return fail(PW_EINVAL, "ring sink: shape mismatch or the chunk does not fit the ring");
    if (sink->episode_return && (!sink->finished_sum || !sink->finished_count || !sink->scratch))
        return fail(PW_EINVAL, "bookkeeping needs episode_return, finished_sum, finished_count and scratch");
    return PW_OK;
}

// The sink into the argument block of a one-launch rollout (its RolloutSink member; the block is zeroed, so without a sink nothing is set).
void sink_into(RolloutSink &K, const pw_rollout_sink *sink)
{
    if (sink && sink->ring) { K.ring = *sink->ring; K.has_ring = 1; K.ring_start = sink->ring_start; }
    if (sink && sink->episode_return) {
        K.episode_return = sink->episode_return; K.finished_sum = sink->finished_sum;
        K.finished_count = sink->finished_count; K.scratch = static_cast<unsigned long long *>(sink->scratch);
    }
}

// Some agent differs from the representative of its role (simple_spread: agent 0; simple_tag: the first adversary / the first good
// agent) in size, sensitivity, force scale or speed clamp -- the test setup_fast_path / setup_tag_path make (pworld.hip).
bool agents_differ_within_role(const KParams &kp)
{
    const int rep[2] = {0, kp.A < kp.N ? kp.A : 0};
    for (int i = 0; i < kp.N; ++i) {
        const int r = rep[i >= kp.A ? 1 : 0];
        if (kp.agent_size[i] != kp.agent_size[r] || kp.agent_sens[i] != kp.agent_sens[r] ||
            kp.agent_fscale[i] != kp.agent_fscale[r] || kp.agent_max_speed[i] != kp.agent_max_speed[r])
            return true;
    }
    return false;
}

}  // namespace
