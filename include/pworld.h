/* pworld.h -- C ABI of libpworld.so: the MI355X (gfx950) batched particle-world.
 *
 * Drop-in boundary for the environment surface the reference drives:
 *   MultiAgentEnv.reset()/step()  call sites  experiments/run.py:28,44,60
 *   make_env() configuration                  experiments/scenarios.py:124-192
 *   local observation layout                  experiments/scenarios.py:6-20
 *   episode length / terminal rule            experiments/run.py:49-50, rls/arglist.py:5
 *   transition sink (replay)                  rls/replay_buffer.py:30-52
 * The arithmetic itself (World.step & friends) lives in the third-party
 * `multiagent` package the reference imports (experiments/scenarios.py:2-3);
 * each entry point names the upstream function it replaces.
 *
 * Conventions
 *   - plain C types only; every pointer marked "device" is caller-owned HBM
 *     (PyTorch allocates it); the library never allocates or frees device memory
 *   - every launch is asynchronous on the caller's hipStream_t (passed as void*,
 *     e.g. torch.cuda.current_stream().cuda_stream); no hidden synchronisation,
 *     so calls are hipGraph-capturable
 *   - return 0 on success, a negative PW_E* code otherwise; pw_last_error() gives
 *     the thread-local message of the last failure
 *   - one handle per (device, env shard); a handle is not thread-safe
 *
 * Layouts (B envs, N agents, L landmarks, D = pw_obs_dim):
 *   state block (device, pw_state_bytes, 256-B aligned planes, SoA over [B x N]):
 *     pos_x[B*N] pos_y[B*N] vel_x[B*N] vel_y[B*N] lm_x[B*L] lm_y[B*L]
 *     ep_step[B] (int32) ep_count[B] (uint32)      -- offsets: pw_state_layout
 *   obs [B,N,D] f32 row-major (rows of ragged simple_tag agents zero-padded)
 *   rew [B,N] f32; done [B,N] u8 (always 0: upstream done_callback is None);
 *   terminal [B] u8 (episode_step >= max_episode_len, run.py:50);
 *   coll [B,N] u64, bit j = is_collision(agent j, agent i) (bit i is always set,
 *   exactly as upstream's reward loop counts it)
 *
 * Reset RNG (device path): Philox4x32-10, counter = (entity, episode, env_id lo,
 *   env_id hi), key = (seed lo, seed hi); entity = agent index, or N + landmark
 *   index; x = out[0], y = out[1]; u = (r >> 8) * 2^-24; value = (hi-lo)*u + lo in
 *   float32 without FMA.  env_id = env_id_base + local env index, so a batch
 *   split over GPUs draws the same states as the unsplit batch.
 *   (The B = 1 compatibility env instead draws from NumPy's global legacy stream on
 *   the host, as upstream reset_world does -- main.py:47 -- and uploads via pw_set_state.)
 *
 * Numerics: IEEE float32, no IMPLICIT FMA contraction, correctly rounded / and sqrt, and
 *   a libm-free deterministic softplus/exp whose polynomial steps are explicit fmaf (definitions:
 *   pworld_math.h, revision 3).  A CPU implementation following pworld_math.h reproduces every
 *   output bit for bit.
 */
#ifndef PWORLD_H
#define PWORLD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PW_VERSION 124 /* 0.1.24: + pw_episode_log_absorb / pw_episode_log_scratch_bytes and pw_episode_log (the per-episode, per-agent returns of a chunk as a log in device memory: one entry per finished episode in (end step, env) order, float64 sums in the order of the reference's loop, no floating-point atomic; translation unit pworld_episode_log.hip, kernels csrc/pw_kernels_episode_log.hpp).  No entry point changed.  0.1.23: + pw_replay_add_wire_agents / pw_replay_add_state_wire_agents / pw_replay_add_ref_wire_agents and pw_wire_agent_rew_bytes (per-agent wire blocks: the per-agent reward plane rew [T,B,N] f32 travels as a trailer behind a wire block of any format, at offset total_bytes, and the learner rank's append writes a per-agent ring -- row ring, STATE ring, simple_reference's two-head ring -- in one launch; the BiCNet baseline trains on several ranks).  No struct, layout or entry point changed: the plain wire entry points keep refusing a per-agent ring.  0.1.22: the ring of pw_rollout_sink may be a per-agent ring (pw_replay_store.per_agent: rew / done [cap,N]) in every form of pw_policy_rollout -- the row ring and the STATE ring of the simple_spread / simple_tag forms, the row ring of the generic form, the two-head ring of simple_reference: every live lane stores its own reward, the value the launch writes to rew[t, env, a], and done = 0; a STATE ring may be per-agent (single head; pw_replay_gather / pw_replay_sample then return out_rew / out_done [b,N]).  The tail / packed / wire entry points keep refusing a per-agent ring.  No entry point changed.  0.1.21: + pw_head_train_forward / pw_head_train_backward / pw_head_train_scratch_bytes (the output layers of the learner's networks with gradient: the ReLU on the actor's BiLSTM output and up to three heads as one launch forward and two backward; a head that received no gradient is passed as NULL and costs nothing; the parameter gradients are summed across workgroups in a fixed order through a caller-provided scratch, without floating-point atomics; translation unit pworld_head.hip, kernels csrc/pw_kernels_head.hpp).  No entry point changed.  0.1.20: + pw_lstm_train_wgrad / pw_lstm_train_wgrad_scratch_bytes (the two recurrent-weight gradients dW_hh of the learner's LSTMs, dG^T against the output shifted by one step, read in place: two launches for both directions, summed across workgroups in a fixed order through a caller-provided scratch, without floating-point atomics; translation unit pworld_lstm_wgrad.hip, kernels csrc/pw_kernels_lstm_wgrad.hpp).  No entry point changed.  0.1.19: the forward ReLU of every network kernel (dense front, attention pooling, the no-gradient critics, every actor form, the one-launch policy rollouts) carries a NaN instead of replacing it by 0, as torch.relu does; every finite input gives the bits it gave before.  No entry point changed.  0.1.18: + pw_front_train_forward / pw_front_train_backward / pw_front_train_scratch_bytes (the dense front of the learner's networks with gradient: dense1, ReLU and the LSTM's input projection as one launch forward and two backward; the parameter gradients are summed across workgroups in a fixed order through a caller-provided scratch, without floating-point atomics; translation unit pworld_front.hip).  No entry point changed.  0.1.17: + pw_gumbel_st_forward / pw_gumbel_st_backward (the learner's hard and soft Gumbel-softmax sample with gradient, one launch each; the noise is the actor heads' Philox draw keyed (seed; step + a device cell, row)).  No entry point changed.  0.1.16: + pw_replay_sample (the batch draw on the device, with or without the gather, numbered and bounded by two device cells), pw_replay_draw_host, pw_adam_step_dev (Adam with the step count in device memory) and pw_adam_bias_scalars: what a captured update needs.  No entry point changed.  0.1.15: + pw_critic_forward_model (the model-learning variant's critic as one launch: no ReLU on the context, Q and the reward prediction from two heads summed in one order, the TD target from the launch's own Q).  0.1.14: + pw_attention_pool_forward / pw_attention_pool_backward (the attention block of the learner's critic with gradient: scores against the last step, softmax over the agent axis, weighted sum, ReLU; one launch each).  0.1.13: the statistics scratch of pw_policy_rollout (pw_rollout_sink.scratch) serves ANY sequence of launch forms on handles of equal num_envs: the ticket word no longer moves with the launch's grid (a launch with fewer workgroups than its predecessor on the same scratch -- pw_dispatch.policy_form changed, pw_actor_set_bf16x3, two handles behind one actor -- dropped its finished episodes).  No entry point changed.  0.1.12: + pw_lstm_train_forward / pw_lstm_train_backward (the recurrent part of a one-layer LSTM with gradient, one launch each, for the learner's passes).  0.1.11: + pw_critic_forward_steps (the BiCNet baseline's per-step critic and per-agent TD target as one launch); pw_replay_add_rollout serves per-agent rings (rew / done planes [cap,N] from io->rew / io->done).  0.1.10: pw_actor_fused and pw_actor_front take observation rows of up to 104 numbers (in_dim in [1, 104]; was 64): pw_actor_fused_kernel / pw_actor_front_kernel at S1C = 9 .. 13.  0.1.9: + the generic one-launch policy rollout (pw_dispatch.policy_form = 5, and automatically for the simple_spread / simple_tag handles the specialised forms refuse: full observation, L > N, landmark contact, force_generic) and pw_policy_generic_envs_per_workgroup.  0.1.8: + pw_adam_step / pw_soft_update (global-norm clip, Adam and the Polyak update of the target network as one launch).  0.1.7: + pw_critic_forward (the learner's critic forward and TD target as one launch).  0.1.6: + STATE rings (pw_replay_store.state_rows: the ring keeps {vel, pos} + the episode's landmarks, pw_replay_gather rebuilds the rows);
                          state-only wire blocks for simple_tag (pw_state_wire_layout_scn), compact-row wire blocks for simple_reference (pw_ref_wire_*); pw_replay_store and pw_state_wire grew (appended fields, zero = before);
                          PWORLD_POLICY_V2 no longer read.  0.1.5: + pw_state_wire_* / pw_replay_add_state_wire (state-only wire blocks); PW_ACTOR_BF16X3 environment switch removed; 0.1.4: + pw_set_actor_precision / pw_actor_set_bf16x3 (opt-in bf16x3 input projection); pw_actor_front_pack's
                          image grew a third section.  0.1.3: + pw_dispatch (kernel selection frozen in the handle; no environment reads at launch)
                          (0.1.2: + pw_rollout_kernel; 0.1.1: pw_replay_store grew act_heads / per_agent / head_width; wire-block entry points) */
#define PW_MAX_AGENTS 64
#define PW_MAX_LANDMARKS 64

enum pw_scenario { PW_SIMPLE_SPREAD = 0, PW_SIMPLE_TAG = 1, PW_SIMPLE_REFERENCE = 2, PW_SIMPLE_SPEAKER_LISTENER = 3 };
#define PW_DIM_C 10   /* simple_reference: world.dim_c communication symbols */
#define PW_SL_DIM_C 3 /* simple_speaker_listener: world.dim_c */
enum pw_obs_mode { PW_OBS_LOCAL = 0, PW_OBS_FULL = 1 };
enum pw_error {
    PW_OK = 0,
    PW_EINVAL = -1,   /* bad argument / unsupported configuration */
    PW_ESTATE = -2,   /* state block not bound */
    PW_EHIP = -3,     /* a HIP runtime call failed (message has hipGetErrorString) */
    PW_ENOMEM = -4
};

typedef struct pw_handle pw_handle;

/* Mirrors what make_env()/make_world() fix for one env (experiments/scenarios.py:124-192)
 * plus the World constants (upstream core.py World.__init__).
 * simple_spread and simple_tag honour every field.  The communication scenarios (simple_reference,
 * simple_speaker_listener) scale both agents' actions by default_sensitivity and have neither a force scale nor a
 * speed clamp: pw_create returns PW_EINVAL when any agent_accel[i] >= 0, any agent_max_speed[i] >= 0 or
 * action_force_uses_accel != 0 (dt, damping, mass and default_sensitivity stay free). */
typedef struct pw_config {
    uint32_t struct_size;            /* = sizeof(pw_config); checked */
    int32_t scenario;                /* pw_scenario */
    int32_t num_envs;                /* B of THIS handle (the local shard) */
    int32_t num_agents;              /* N <= PW_MAX_AGENTS */
    int32_t num_landmarks;           /* L <= PW_MAX_LANDMARKS */
    int32_t num_adversaries;         /* simple_tag: agents [0, A) are adversaries */
    int32_t obs_mode;                /* pw_obs_mode (simple_spread only) */
    int32_t max_episode_len;         /* rls/arglist.py:5 (25); 0 = never terminal */
    int32_t auto_reset;              /* reset an env inside the step that made it terminal (run.py:59-60) */
    int32_t force_discrete_action;   /* experiments/scenarios.py:191; applies to act_vec input */
    int32_t landmark_collide;        /* simple_spread 0, simple_tag 1 */
    int32_t action_force_uses_accel; /* fork knob: p_force = mass*accel*u; canonical 0 */
    uint64_t seed;                   /* Philox key */
    uint64_t env_id_base;            /* global index of local env 0 (multi-GPU sharding) */
    float dt, damping, contact_force, contact_margin, default_sensitivity, mass, landmark_size;
    float agent_size[PW_MAX_AGENTS];
    float agent_accel[PW_MAX_AGENTS];     /* < 0: None (sensitivity = default_sensitivity) */
    float agent_max_speed[PW_MAX_AGENTS]; /* < 0: None */
} pw_config;

typedef struct pw_state_layout {
    size_t pos_x, pos_y, vel_x, vel_y, lm_x, lm_y, ep_step, ep_count; /* byte offsets */
    size_t total_bytes;
    size_t comm, goal; /* communication scenarios only: state.c [B*N*dim_c] f32 (dim_c = PW_DIM_C for simple_reference,
                          PW_SL_DIM_C for simple_speaker_listener), goal_b index [B*N] i32 */
} pw_state_layout;

/* Buffers of one step (T = 1) or of a T-step rollout (leading dimension T).
 * Any output pointer may be NULL (that output is skipped). Exactly one of
 * act_idx / act_vec is non-NULL. All pointers are device pointers. */
typedef struct pw_step_io {
    const int32_t *act_idx; /* [T,B,N] action index 0..4 (0 noop,1 +x,2 -x,3 +y,4 -y) */
    const float *act_vec;   /* [T,B,N,5] one-hot / soft action, as run.py:38 passes it */
    float *obs;             /* [T,B,N,D] what the policy sees next (post-reset where auto-reset fired) */
    float *final_obs;       /* [T,B,N,D] pre-reset observation; written only for envs that reset */
    float *rew;             /* [T,B,N] per-agent reward (world.collaborative = False) */
    float *rew_shared;      /* [T,B]   sum over agents in agent order (run.py:46) */
    uint8_t *done;          /* [T,B,N] always 0 */
    uint8_t *terminal;      /* [T,B] */
    uint64_t *coll;         /* [T,B,N] */
    const int32_t *act_comm; /* [T,B,N] communication symbol 0..PW_DIM_C-1; simple_reference with act_idx.
                                There act_vec is [T,B,N,5+PW_DIM_C]: the concatenated MultiDiscrete action of
                                experiments/run.py:39-41 (movement one-hot | communication vector).
                                simple_speaker_listener has one action head per agent (upstream environment.py:
                                Discrete(3) for the speaker, Discrete(5) for the listener): act_idx [T,B,N] =
                                (symbol 0..2 of agent 0, movement 0..4 of agent 1), or act_vec [T,B,N,5] with the
                                speaker's vector in the first three entries; act_comm stays NULL */
} pw_step_io;

int pw_version(void);
const char *pw_last_error(void);

/* Canonical upstream constants for a scenario: simple_spread (N agents, L = N
 * landmarks), simple_tag (num_adversaries + good, L = 2), simple_reference (2 speaking agents, L = 3;
 * obs = [p_vel, landmark - pos, goal_b colour, other agent's c], D = 21) or simple_speaker_listener (a fixed
 * speaker + a silent moving listener, L = 3; obs = [p_vel, landmark - pos, goal_b colour or zeros], D = 11, the
 * observation experiments/scenarios.py:45-64 patches in). Replaces Scenario.make_world() + World.__init__(). */
int pw_config_default(pw_config *cfg, int scenario, int num_envs, int num_agents,
                      int num_landmarks /* <0: scenario default */, int num_adversaries);

int pw_create(const pw_config *cfg, pw_handle **out); /* MultiAgentEnv.__init__ */
void pw_destroy(pw_handle *h);
int pw_obs_dim(const pw_handle *h);                   /* observation_space[i].shape[0] */
int pw_get_config(const pw_handle *h, pw_config *out);
/* env.force_discrete_action = ... after construction (experiments/scenarios.py:191) */
int pw_set_force_discrete_action(pw_handle *h, int on);
int pw_get_state_layout(const pw_handle *h, pw_state_layout *out);
size_t pw_state_bytes(const pw_handle *h);
int pw_bind_state(pw_handle *h, void *device_state_block);

/* AoS <-> SoA: pos/vel [B,N,2], lm [B,L,2] f32 device (upstream p_pos / p_vel arrays);
 * ep_step/ep_count [B] may be NULL (set: zeroed / get: skipped), each on its own: a set with ep_step alone keeps
 * the steps and zeroes ep_count, and the other way round.  pos, vel and lm may each be NULL as well: a set leaves
 * that part of the state as it is (a set with all five NULL only zeroes the counters), a get skips it
 * (tests/test_gpu_aux_entry_points.py). */
int pw_set_state(pw_handle *h, const float *pos, const float *vel, const float *lm,
                 const int32_t *ep_step, const uint32_t *ep_count, void *stream);
int pw_get_state(pw_handle *h, float *pos, float *vel, float *lm,
                 int32_t *ep_step, uint32_t *ep_count, void *stream);

/* Communication scenarios only: the communication state (agent.state.c, [B,N,dim_c] f32) and each agent's goal
 * landmark index (goal_b, [B,N] i32; the listener's entry is unused).  Either pointer may be NULL. */
int pw_set_comm_state(pw_handle *h, const float *comm, const int32_t *goal, void *stream);
int pw_get_comm_state(pw_handle *h, float *comm, int32_t *goal, void *stream);

/* MultiAgentEnv.reset(): env_mask [B] u8 device or NULL (= all). Masked-in envs get
 * ep_count += 1, ep_step = 0, Philox initial state; obs (may be NULL) is written for ALL envs. */
int pw_reset(pw_handle *h, const uint8_t *env_mask, float *obs, void *stream);
/* scenario.observation for every agent from the current state. */
int pw_observe(pw_handle *h, float *obs, void *stream);
/* scenario.reward / is_collision from the current state (no step).  rew or coll may be NULL (both: PW_EINVAL); the
 * communication scenarios have no collisions and take coll = NULL only (PW_EINVAL otherwise). */
int pw_reward(pw_handle *h, float *rew, uint64_t *coll, void *stream);

/* MultiAgentEnv.step(): _set_action, World.step (apply_action_force,
 * apply_environment_force/get_collision_force, integrate_state), then per agent
 * observation, reward, done -- one fused launch for all B envs. */
int pw_step(pw_handle *h, const pw_step_io *io, void *stream);
/* T consecutive steps in ONE launch (state stays in registers/LDS between steps). */
int pw_rollout(pw_handle *h, const pw_step_io *io, int num_steps, void *stream);

/* ---- kernel selection ------------------------------------------------------------------------------------------
 * The dispatcher picks a kernel form per (scenario, N, L, B, outputs requested) from measured crossovers.  Every field
 * below overrides one of those choices for ONE handle; the selection lives in the handle, is fixed by pw_create /
 * pw_set_dispatch, and nothing on the pw_step / pw_rollout / pw_policy_rollout path reads the process environment.
 * pw_create initialises it from pw_dispatch_default() overlaid, once, with the PWORLD_* environment variables of the
 * creating process (for A/B runs of unmodified host programs: PWORLD_FORCE_GENERIC, PWORLD_NO_STREAM, PWORLD_NO_DUO,
 * PWORLD_FORCE_DUO, PWORLD_NO_QUAD, PWORLD_FORCE_QUAD, PWORLD_OBS_BLOCK, PWORLD_SPREAD_TRIO / PWORLD_TAG_TRIO,
 * PWORLD_P_PRIO, PWORLD_EPW, PWORLD_POLICY_V3 / PWORLD_POLICY_V3J); pw_set_dispatch replaces it.  Results never depend
 * on it: every form produces the same bits (tests/test_gpu_parity.py runs them all against the oracle). */
typedef struct pw_dispatch {
    uint32_t struct_size;  /* = sizeof(pw_dispatch); checked */
    int32_t force_generic; /* 1: the generic kernel (pw_rollout_kernel) for every launch */
    int32_t no_stream;     /* 1: no streaming family (quad / duo / stream): pw_spread_fast_kernel, generic simple_tag */
    int32_t duo;           /* -1 auto (by grid size); 0: the one-wave stream form (and no quad form); 1: the two-wave duo form on any grid */
    int32_t quad;          /* -1 auto; 0: off; 1: pw_spread_quad_kernel wherever it applies (N = L = 6, unit mass) */
    int32_t obs_block;     /* -1 auto; 0: row-wise observation stores; 1: block-wise */
    int32_t trio;          /* -1 auto; 0 / 1: the three-wave variants of the duo kernels (spread: block-store forms, N >= 6) */
    int32_t p_prio;        /* -1 auto; >= 0: issue-priority bits of the duo kernels' waves (2 bits per wave; simple_tag: 0 / 1) */
    int32_t envs_per_wave; /* 0 auto; n >= 1: envs per wave, clamped to 64 / N */
    int32_t policy_form;   /* 0 auto; 3: pw_policy_rollout3_kernel; 4: pw_policy_rollout3j_kernel; 1, 2: retired (PW_EINVAL)
                            * (the third form with dense1 just in time: long agent axes, N <= 32);
                            * 5: pw_policy_rollout_generic_kernel on any simple_spread / simple_tag handle it fits */
} pw_dispatch;
int pw_dispatch_default(pw_dispatch *d);                    /* every choice automatic */
int pw_set_dispatch(pw_handle *h, const pw_dispatch *d);    /* between launches; the bound state is untouched */
int pw_get_dispatch(const pw_handle *h, pw_dispatch *out);

/* Arithmetic of the actor inside the one-launch policy rollouts of this handle (pw_policy_rollout).  PW_ACTOR_F32 (default): exact
 * float32, bit-identical to every other form and to the pw_actor_fused + pw_step loop.  PW_ACTOR_BF16X3: OPT-IN and NOT exact -- the
 * LSTM input projection runs on bfloat16 matrix instructions with both operands split in high and low halves, three products per k
 * step, float32 accumulation; dense1, the recurrence and the head stay float32.  Within the 2e-5 bound of the PyTorch float32
 * comparison on the reference's weights (tests/test_gpu_engine.py), but sampled actions can differ from the exact form's.
 * Selected by this call only (no environment variable changes results: a process-wide switch would silently turn every "exact"
 * rollout of the process into this mode); never a default, never a headline figure.
 * Served by the simple_spread rollout in its third kernel form and by pw_actor_fused at N <= 16 with rows of at most 64 numbers;
 * anything else returns PW_EINVAL rather than run in float32 unannounced.
 * pw_actor_set_bf16x3: the same switch for the handle-less pw_actor_fused (process-wide, off until set; N <= 16 and in_dim <= 64
 * only: rows of 65 .. 104 numbers run on pw_actor_fused_kernel, which has no bf16x3 form). */
#define PW_ACTOR_F32 0
#define PW_ACTOR_BF16X3 1
int pw_set_actor_precision(pw_handle *h, int32_t mode);
int pw_get_actor_precision(const pw_handle *h);
int pw_actor_set_bf16x3(int32_t on);   /* returns the previous value */

/* Name of the device kernel the last pw_step / pw_rollout / pw_policy_rollout on this handle launched (a static string; "" before the
 * first launch).  The dispatcher picks a kernel per (scenario, N, L, B, outputs requested): measurement tools name the
 * dominant kernel from this, not from a table of their own. */
const char *pw_rollout_kernel(const pw_handle *h);

/* Algorithmic HBM bytes of one env-step (SURVEY.md 8(d)): 57N + 8L + 8NL for local obs. */
size_t pw_algorithmic_bytes_per_env_step(const pw_handle *h);

/* ---- device replay ring (rls/replay_buffer.py:9-91 ReplayBuffer) -----------------
 * Storage is caller-owned SoA: obs/next_obs [cap,N,D] f32, act [cap,N] u8 index,
 * rew [cap] f32 (shared reward), done [cap] f32.
 * Variants (zero = the plain ring above, so a memset struct keeps its old meaning):
 *   act_heads = 2: act is [cap,N,2] u8 = (movement, communication symbol) -- the MultiDiscrete action of
 *     experiments/run.py:39-41; head_width = {5, dim_c} sizes the one-hot rows pw_replay_gather returns
 *     (head_width[0] = 0 means 5);
 *   per_agent = 1: rew and done are [cap,N] f32 -- the BiCNet tuple of experiments/run_BIC.py:46,50.
 * pw_replay_add, pw_replay_add_rollout, pw_replay_gather and pw_replay_sample serve every variant of the row ring.  The
 * pw_policy_rollout sink (0.1.22) takes the single-head ring on simple_spread / simple_tag and the two-head ring on simple_reference,
 * each with the shared reward or per-agent.  The tail / packed / wire entry points (pw_replay_add_tail, pw_replay_add_packed,
 * pw_replay_add_wire, pw_replay_add_state_wire, pw_replay_add_ref_wire) take the shared-reward ring only: their blocks carry the
 * shared reward (PW_EINVAL otherwise).  The per-agent ring's wire entry points (0.1.23) are pw_replay_add_wire_agents,
 * pw_replay_add_state_wire_agents and pw_replay_add_ref_wire_agents: the same blocks with the per-agent reward plane behind them
 * (pw_wire_agent_rew_bytes); they take the per-agent ring only (PW_EINVAL for a shared-reward ring).
 *   state_rows = 1 (0.1.6): a STATE ring.  obs / next_obs are [cap,N,4] f32 planes holding {vx, vy, px, py} of every agent (the
 *     first four columns of its observation row) and lm [cap,L,2] the landmarks of the transition's episode: 32N + 8L bytes per
 *     transition instead of 8ND (C2: 240 instead of 768) -- what the learner rank writes per gathered transition.  obs_dim stays D:
 *     pw_replay_gather REBUILDS the rows it returns ([b,N,D]; every entry is the state itself or one float32 subtraction, so the
 *     batch is bit-identical to the row ring's).  scenario / num_landmarks / num_adversaries name the row layout: PW_SIMPLE_SPREAD
 *     with the local observation (D = 4 + 2L) or PW_SIMPLE_TAG (D = 4 + 2L + 2(N - 1) + 2(N - A), good agents' rows zero-padded).
 *     Filled by pw_replay_add_state_wire and by the pw_policy_rollout ring sink (which hold the state itself); the writers that are
 *     handed ROWS return PW_EINVAL (a row cannot be turned back into the landmarks it was built from).  Single-head rings only.  0.1.22: per_agent = 1 is served
 *     -- rew / done [cap,N], filled by the pw_policy_rollout sink and (0.1.23) by pw_replay_add_state_wire_agents, which reads the
 *     per-agent reward plane behind the block (pw_replay_add_state_wire itself returns PW_EINVAL: the block carries the shared
 *     reward); pw_replay_gather / pw_replay_sample return out_rew / out_done [b,N] and the rows of the shared STATE ring. */
typedef struct pw_replay_store {
    float *obs, *next_obs, *rew, *done;
    uint8_t *act;
    int64_t capacity;
    int32_t num_agents, obs_dim;
    int32_t act_heads, per_agent;
    int32_t head_width[2];
    int32_t state_rows, num_landmarks, scenario, num_adversaries; /* 0.1.6; all zero = the row ring of before */
    float *lm;                                                    /* state ring: [cap,L,2] */
} pw_replay_store;

/* add(): append B transitions at ring positions (start + i) % capacity.
 * next_obs row i comes from final_obs where terminal[i] != 0 (and final_obs != NULL).
 * act_idx is [B,N] int32 ([B,N,2] when st->act_heads = 2); rew_shared / done are [B] ([B,N] when st->per_agent). */
int pw_replay_add(const pw_replay_store *st, int64_t start, const int64_t *start_dev /* device, or NULL */,
                  int32_t B, const float *obs, const int32_t *act_idx, const float *rew_shared,
                  const float *next_obs, const float *final_obs, const uint8_t *terminal,
                  const float *done /* [B] or NULL = 0 */, void *stream);
/* hipGraph support: a captured launch freezes by-value arguments; the two values that change every
 * step (ring position, Philox step) can instead live in device memory (start_dev / step_dev override the
 * by-value argument when non-NULL) and be advanced by this one-thread launch inside the same graph:
 * *counter = (*counter + delta) % modulo (modulo <= 0: no wrap). */
int pw_counter_add(int64_t *counter, int64_t delta, int64_t modulo, void *stream);
/* sample_index() / _encode_sample(): gather rows idx[0..b) into dense batch tensors;
 * out_act is one-hot f32 [b,N,5] exactly as the reference's trainer consumes it ([b,N,head_width[0]+head_width[1]]
 * for a two-head ring); out_rew / out_done are [b] ([b,N] for a per-agent ring).  (Declared below.) */
/* pw_replay_add + pw_episode_stats in ONE launch (the last launch of a captured rollout step).  The ring
 * position comes from `start` or, if non-NULL, *start_dev; (position + B) % capacity is written to
 * *next_start_dev (optional; must not alias start_dev: double-buffer the cursor) and *step_counter (optional,
 * e.g. the policy's Philox step) is incremented.  Episode-return arithmetic is identical to pw_episode_stats. */
int pw_replay_add_tail(const pw_replay_store *st, int64_t start, const int64_t *start_dev, int64_t *next_start_dev,
                       int32_t B, const float *obs, const int32_t *act_idx, const float *rew_shared,
                       const float *next_obs, const float *final_obs, const uint8_t *terminal, const float *done,
                       float *episode_return, double *finished_sum, int64_t *finished_count, int64_t *step_counter,
                       void *stream);
/* A whole rollout chunk (pw_policy_rollout / pw_rollout outputs, [T, ...]) into the ring in one launch: transition
 * (t, e) goes to slot (start + t*B + e) % capacity -- the order of T pw_replay_add calls -- with obs = obs0 [B,N,D]
 * for t = 0 and the chunk's obs[t-1] after that, next_obs = final_obs where terminal.  io needs obs, rew_shared,
 * terminal (final_obs optional; a per-agent ring, st->per_agent: also rew [T,B,N], required, and done [T,B,N] u8 or NULL = 0, which
 * fill its [cap,N] planes -- the bookkeeping stays on rew_shared); act [T,B,N] int32 ([T,B,N,2] for a two-head ring, st->act_heads = 2: the MultiDiscrete chunks
 * of pw_policy_rollout on simple_reference).  episode_return / finished_sum / finished_count / scratch
 * (all or none): the chunk's episode-return bookkeeping, as T pw_episode_stats calls up to float64 summation
 * order (fixed, so reproducible); scratch = pw_replay_add_rollout_scratch_bytes(B) device bytes, zeroed once.
 * Like pw_replay_add and pw_replay_gather it refuses (PW_EINVAL) st->act_heads outside [0, 2] and a two-head ring whose
 * head_width[0] < 0 or head_width[1] < 1: it used to take act_heads = 3 and store one index per agent where the gather reads two. */
int pw_replay_add_rollout(const pw_replay_store *st, int64_t start, int32_t B, int32_t T, const float *obs0,
                          const pw_step_io *io, const int32_t *act, float *episode_return, double *finished_sum,
                          int64_t *finished_count, void *scratch, void *stream);
size_t pw_replay_add_rollout_scratch_bytes(int32_t B);
int pw_replay_gather(const pw_replay_store *st, const int64_t *idx, int32_t b,
                     float *out_obs, float *out_act, float *out_rew, float *out_next_obs,
                     float *out_done, void *stream);
/* make_index() + sample_index() as ONE launch whose every changing input lives in device memory (a captured launch freezes by-value
 * arguments): draws b ring slots and, where outputs are given, gathers them exactly as pw_replay_gather would (row, two-head,
 * per-agent and STATE rings; the same arithmetic, so the same bits as pw_replay_gather on out_idx).
 *   c = *call_dev (which draw this is), len = clamp(*len_dev, 1, st->capacity) (how many transitions the ring holds);
 *   element e takes word (e & 3) of Philox4x32-10(counter = (e >> 2, c lo, c hi, 0x52504C59), key = (seed lo, seed hi));
 *   idx = ((u64)word * (u64)len) >> 32.
 * Uniform with replacement up to a relative bias of len / 2^32 (2.3e-4 at 10^6 transitions; torch.randint's modulo has the same kind).
 * The clamp makes an out-of-range slot impossible whatever the cell holds; an empty ring is the caller's to refuse.  The counter
 * domain meets neither the reset draws nor the Gumbel noise (csrc/pw_replay_draw.hpp lists the streams).  The launch does not
 * advance *call_dev: follow it with pw_counter_add(call_dev, 1, 0, stream).  out_idx [b] (optional) receives the slots; out_idx
 * alone, every other output NULL, is the draw alone (make_index).  PW_EINVAL, nothing launched: a null st, call_dev or len_dev,
 * b < 1, all six outputs NULL, a capacity above 2^32 -- and what pw_replay_gather refuses. */
int pw_replay_sample(const pw_replay_store *st, uint64_t seed, const int64_t *call_dev, const int64_t *len_dev, int32_t b,
                     int64_t *out_idx /* may be NULL */, float *out_obs, float *out_act, float *out_rew,
                     float *out_next_obs, float *out_done /* each may be NULL */, void *stream);
/* The draw of pw_replay_sample on the host: the slot of element e of draw number `call` at length len (clamped to [1, 2^32]). */
int64_t pw_replay_draw_host(uint64_t seed, int64_t call, int64_t e, int64_t len);

/* ---- multi-GPU exchange (one rank per GPU; the collective itself is RCCL, driven by the host) ----
 * A transition row is f32 [obs N*D | next_obs N*D | act N | rew | done], width 2*N*D + N + 2.
 * pw_pack_transitions: row r = transition (sel_t[r] >= 1, sel_e[r]) of a T-step chunk described by
 * io (obs[t-1] is the observation acted on; next_obs is final_obs where terminal, else obs[t]).
 * pw_replay_add_packed: ReplayBuffer.add() of R received rows at ring positions (start + r) % capacity. */
int pw_pack_transitions(const pw_step_io *io, int32_t B, int32_t N, int32_t D, const int32_t *sel_t,
                        const int32_t *sel_e, int32_t R, float *rows, void *stream);
int pw_replay_add_packed(const pw_replay_store *st, int64_t start, int32_t R, const float *rows, void *stream);
/* Both of the above in ONE launch (either half may be disabled: st/rows_in NULL or io/rows_out NULL):
 * append the R_in rows of the previous collective to the ring, pack R_out rows of this chunk for the next. */
int pw_exchange(const pw_replay_store *st, int64_t start, int32_t R_in, const float *rows_in, const pw_step_io *io,
                int32_t B, int32_t N, int32_t D, const int32_t *sel_t, const int32_t *sel_e, int32_t R_out,
                float *rows_out, void *stream);

/* ---- full gather of transitions to the learner rank (north_star: "RCCL-over-xGMI gather of transitions into
 * rls/replay_buffer"; consumer experiments/run.py:20-21,52) ------------------------------------------------------
 * One WIRE BLOCK per rank per T-step rollout chunk carries EVERY transition of the chunk once: the observation
 * is sent once per step (next_obs of step t is obs of step t+1), plus the pre-reset observation only for the steps
 * that ended an episode (run.py:52 stores new_obs_n BEFORE env.reset(), :60).  Planes, 256-B aligned:
 *   obs0 [B,N,D] f32        observation the policy acted on at step 0
 *   obs [T,B,N,D] f32       post-step (post-reset) observations -- the rollout kernels write them HERE, no copy
 *   final_rows [F,B,N,D] f32  pre-reset observation of env e's k-th episode end inside the chunk,
 *                           F = ceil(T / max_episode_len) (0 when episodes never end)
 *   rew_shared [T,B] f32    written in place by the rollout as well
 *   act [T,B,N] u8          action index
 *   fin_slot [T,B] u8       k where step (t, e) ended an episode, 0xFF elsewhere
 * = N*D*4 + N + 5 bytes per env-step (C2: 395 B, SURVEY.md 8(e)) + (1 + F) observation batches per chunk (C2,
 * T = 100: 414 B/env-step in all).
 * The collective itself is RCCL, driven by the host: direct peer -> root sends, one block per peer per chunk. */
typedef struct pw_chunk_wire {
    int32_t T, B, N, D, F, reserved;
    size_t obs0, obs, final_rows, rew_shared, act, fin_slot; /* byte offsets into the block */
    size_t total_bytes;
} pw_chunk_wire;
int pw_chunk_wire_layout(int32_t T, int32_t B, int32_t N, int32_t D, int32_t max_episode_len, pw_chunk_wire *out);
/* Sender, after the chunk's rollout wrote obs / rew_shared into the block: fills obs0, final_rows, act, fin_slot
 * from obs0 [B,N,D], the rollout's dense final_obs [T,B,N,D] (may be NULL when F = 0), terminal [T,B] and
 * act [T,B,N] int32.  One launch. */
int pw_chunk_wire_finalize(const pw_chunk_wire *w, void *wire, const float *obs0, const float *final_obs,
                           const uint8_t *terminal, const int32_t *act, void *stream);
/* Root: ReplayBuffer.add() of the block's T*B transitions; transition (t, e) goes to ring slot
 * (start + t*B + e) % capacity -- the order T pw_replay_add calls would have used -- bit-identical to
 * pw_replay_add_rollout on the sender's buffers.  One launch. */
int pw_replay_add_wire(const pw_replay_store *st, int64_t start, const pw_chunk_wire *w, const void *wire, void *stream);

/* ---- the same gather on a diet: STATE-ONLY wire blocks (simple_spread, local observation) ---------------------------
 * A local observation row is a pure function of the agent's {vel, pos} and the episode's landmarks
 * (experiments/scenarios.py:6-20: [p_vel, p_pos, landmark.p_pos - p_pos ...]); each entry is ONE float32 operation, so the
 * root can rebuild obs / next_obs rows bit for bit from 16 bytes per agent instead of receiving 4 + 2L floats per agent
 * (C2: 384 B of the 395 B per env-step of the row block above).  Planes, 256-B aligned:
 *   state0 [B,N] float4 {vx, vy, px, py}      the state the policy acted on at step 0 (written by pw_state_wire_begin)
 *   state [T,B,N] float4                      post-step (post-reset) state = columns 0..3 of the rollout's obs rows
 *   final_state [F,B,N] float4                pre-reset state of env e's k-th episode end inside the chunk
 *   lm [(F+1),B,L] float2                     landmarks of the episode in progress at step 0 (k = 0, copied from the state
 *                                             block by pw_state_wire_begin) and after the k-th reset (k >= 1: re-derived by
 *                                             pw_state_wire_finalize from the reset's Philox key (seed, global env id,
 *                                             episode number) -- the in-kernel auto-reset draws exactly these)
 *   ep0 [B] u32                               episode number of every env at step 0 (pw_state_wire_begin; sender-side only,
 *                                             it travels with the block and lets the root audit the landmark planes)
 *   rew_shared [T,B] f32                      written in place by the rollout
 *   act [T,B,N] u8
 *   epi [T,B] u8                              bits 0..6: k = episode ends of env e before step t (which lm / final_state
 *                                             plane applies), bit 7: step (t, e) ended an episode
 * = 17N + 5 bytes per env-step + (1 + F) state and landmark batches per chunk (C2, T = 100: 107 + 7 = 114 B per
 * env-step, 28 % of the row block's 414).
 * Sender:  pw_state_wire_begin (BEFORE the chunk's rollout launch, same stream)  ->  rollout with rew_shared pointing into
 * the block  ->  pw_state_wire_finalize.  Root: pw_replay_add_state_wire = ReplayBuffer.add() of the block's T*B transitions,
 * bit-identical to pw_replay_add_rollout on the sender's buffers (tests/test_gpu_engine.py). */
typedef struct pw_state_wire {
    int32_t T, B, N, L, D, F;
    size_t state0, state, final_state, lm, ep0, rew_shared, act, epi; /* byte offsets into the block */
    size_t total_bytes;
    int32_t scenario, num_adversaries; /* 0.1.6: PW_SIMPLE_SPREAD (0: as before) or PW_SIMPLE_TAG with A adversaries */
} pw_state_wire;
/* Host arithmetic only (as pw_chunk_wire_layout).  begin / finalize return PW_EINVAL unless h is a handle of the block's scenario,
 * B, N, L (and A) whose rows are a function of the state: simple_spread with the local observation (D = 4 + 2L), or simple_tag
 * (0.1.6; D = 4 + 2L + 2(N - 1) + 2(N - A): [vel, pos, landmark - pos .., other pos - pos .., other good agents' vel ..], rows of good
 * agents zero-padded; landmarks drawn from U(-0.9, 0.9): C3's 4 + 2 roster ships 17N + 5 = 107 B per env-step + (1 + F) state /
 * landmark batches per chunk instead of the row block's 4ND + N + 5 = 539). */
int pw_state_wire_layout(int32_t T, int32_t B, int32_t N, int32_t L, int32_t max_episode_len, pw_state_wire *out); /* simple_spread */
int pw_state_wire_layout_scn(int32_t scenario, int32_t T, int32_t B, int32_t N, int32_t L, int32_t num_adversaries,
                             int32_t max_episode_len, pw_state_wire *out);
int pw_state_wire_begin(const pw_handle *h, const pw_state_wire *w, void *wire, void *stream);
/* obs [T,B,N,D] and final_obs [T,B,N,D] (may be NULL when F = 0) are the rollout's outputs, terminal [T,B], act [T,B,N]
 * int32.  One launch. */
int pw_state_wire_finalize(const pw_handle *h, const pw_state_wire *w, void *wire, const float *obs, const float *final_obs,
                           const uint8_t *terminal, const int32_t *act, void *stream);
/* Root; needs no handle: the rebuild is the observation's own arithmetic on the block's data.  One launch.  st may be a row ring
 * (rows rebuilt here) or a STATE ring of the same scenario / N / L / A (states and landmarks copied; rows rebuilt by
 * pw_replay_gather when a batch is sampled). */
int pw_replay_add_state_wire(const pw_replay_store *st, int64_t start, const pw_state_wire *w, const void *wire, void *stream);

/* ---- the gather for simple_reference (the MultiDiscrete scenario of main.py:24,52-54; 0.1.6): COMPACT-ROW wire blocks ------------
 * Its 21-number row is [p_vel (2), landmark - p_pos (3 x 2), goal_b colour (3), the other agent's communication state (10)]
 * (experiments/scenarios.py:23-42).  The last 13 numbers are not arithmetic at all: the colour is a constant of the agent's goal
 * landmark (fixed for an episode) and the communication state is the one-hot of the symbol the OTHER agent sampled in this step
 * (zeros after a reset; upstream update_agent_state copies action.c for a speaking agent).  So a block carries the first EIGHT
 * numbers of every row as they are (the position itself is not in the row, and landmark - pos cannot be turned back into it), one
 * goal byte per agent and episode, and both action heads as bytes; the root rebuilds obs / next_obs bit for bit.  Planes, 256-B aligned:
 *   head0 [B,2,8] f32         columns 0..7 of the rows the policy acted on at step 0
 *   head [T,B,2,8] f32        columns 0..7 of the post-step (post-reset) rows
 *   final_head [F,B,2,8] f32  columns 0..7 of the pre-reset rows of env e's k-th episode end inside the chunk
 *   goal [(F+1),B,2] u8       goal landmark of each agent in the episode in progress at step 0 (k = 0) and after the k-th reset
 *   comm0 [B,2] u8            the symbol visible in agent a's row at step 0 (0xFF: none, i.e. zeros)
 *   rew_shared [T,B] f32      written in place by the rollout
 *   act [T,B,2,2] u8          (movement, symbol) of every agent
 *   epi [T,B] u8              as in pw_state_wire
 * = 73 bytes per env-step + (1 + F) head / goal batches per chunk (T = 100: 77 B; the row block: 181).
 * Sender: pw_ref_wire_finalize after the chunk's rollout (rew_shared pointing into the block); it reads the rollout's outputs only
 * (no handle).  Root: pw_replay_add_ref_wire into the TWO-HEAD ring (act_heads = 2, head widths 5 | PW_DIM_C), bit-identical to
 * pw_replay_add_rollout on the sender's buffers.  The rows must come from HARD symbol indices (pw_policy_rollout, or pw_rollout with
 * act_idx / act_comm): a soft communication vector (act_vec) is not representable -- use pw_chunk_wire_* then. */
typedef struct pw_ref_wire {
    int32_t T, B, F, reserved;
    size_t head0, head, final_head, goal, comm0, rew_shared, act, epi; /* byte offsets into the block */
    size_t total_bytes;
} pw_ref_wire;
int pw_ref_wire_layout(int32_t T, int32_t B, int32_t max_episode_len, pw_ref_wire *out);
/* obs0 [B,2,21], obs / final_obs [T,B,2,21] (final_obs may be NULL when F = 0), terminal [T,B], act [T,B,2,2] int32.  One launch. */
int pw_ref_wire_finalize(const pw_ref_wire *w, void *wire, const float *obs0, const float *obs, const float *final_obs,
                         const uint8_t *terminal, const int32_t *act, void *stream);
int pw_replay_add_ref_wire(const pw_replay_store *st, int64_t start, const pw_ref_wire *w, const void *wire, void *stream);

/* ---- per-agent wire blocks (0.1.23): the gather for a per-agent ring (pw_replay_store.per_agent; the BiCNet tuple) -------------------
 * The three block structs above keep their bytes.  The per-agent reward travels as a TRAILER PLANE behind the block:
 *   rew [T,B,N] f32         at offset w->total_bytes (a multiple of 256) of a block of any format; the rollout writes it in place
 *                           (pw_step_io.rew pointing there), as it writes rew_shared into the block
 * so a per-agent block is w->total_bytes + pw_wire_agent_rew_bytes(T, B, N) bytes: 4N more per env-step (state blocks: 21N + 5
 * instead of 17N + 5).  The sender's calls are the ones above (layout, begin, finalize); nothing else is launched there. */
/* bytes of the per-agent reward plane rew [T,B,N] f32 that follows a wire block of any format at offset
 * w->total_bytes (a multiple of 256), rounded up to 256; 0 sizes are PW_EINVAL-style 0 */
size_t pw_wire_agent_rew_bytes(int32_t T, int32_t B, int32_t N);
/* Root: pw_replay_add_wire / pw_replay_add_state_wire / pw_replay_add_ref_wire for a PER-AGENT ring, one launch each.  Transition
 * (t, e) goes to slot (start + t*B + e) % capacity; obs / next_obs / act (and a STATE ring's lm) are written exactly as the plain
 * entry point writes them; st->rew[slot*N + a] = rew_agents[(t*B + e)*N + a] and st->done[slot*N + a] = 0 (these scenarios have no
 * done callback: what the pw_policy_rollout sink stores).  rew_agents is a device pointer to [T,B,N] f32 -- wire + w->total_bytes
 * in the layout above, or wherever a C host keeps the plane; the block's rew_shared plane is not read.  Served: the row ring from
 * row blocks, the row ring and the STATE ring from state blocks, simple_reference's two-head ring from its compact rows.
 * PW_EINVAL, nothing launched: a ring with per_agent == 0 (use the plain entry point), a null or misaligned rew_agents, and
 * everything the plain entry point refuses (shape or scenario mismatch, a chunk larger than the ring, a two-head ring for a
 * single-head block and the reverse). */
int pw_replay_add_wire_agents(const pw_replay_store *st, int64_t start, const pw_chunk_wire *w, const void *wire,
                              const float *rew_agents, void *stream);
int pw_replay_add_state_wire_agents(const pw_replay_store *st, int64_t start, const pw_state_wire *w, const void *wire,
                                    const float *rew_agents, void *stream);
int pw_replay_add_ref_wire_agents(const pw_replay_store *st, int64_t start, const pw_ref_wire *w, const void *wire,
                                  const float *rew_agents, void *stream);

/* Episode bookkeeping of the rollout loop (experiments/run.py:55-65) over B envs in one launch:
 * episode_return[b] += rew_shared[b]; where terminal[b]: *finished_sum += return (double),
 * *finished_count += 1, return cleared.  Deterministic (single workgroup, fixed-order reduction). */
int pw_episode_stats(const float *rew_shared, const uint8_t *terminal, int32_t B, float *episode_return,
                     double *finished_sum, int64_t *finished_count, void *stream);
/* pw_episode_stats that also advances up to two device-side counters (NULL to skip; value = (value + delta) %
 * modulo, modulo 0 = no wrap) -- e.g. the replay ring cursor and the policy's Philox step of a captured
 * rollout step, whose earlier launches have all read them by the time this one runs (stream order). */
int pw_rollout_tail(const float *rew_shared, const uint8_t *terminal, int32_t B, float *episode_return,
                    double *finished_sum, int64_t *finished_count, int64_t *counter0, int64_t delta0, int64_t modulo0,
                    int64_t *counter1, int64_t delta1, int64_t modulo1, void *stream);

/* ---- action producer (rls/model/ac_network_multi_gumbel.py:24-67, ddpg_gumbel_fix.py:86-116) --------
 * The actor is Linear(D,64)-ReLU-BiLSTM(64->2x32 over the AGENT axis)-ReLU-Linear(64,5).  The two input
 * GEMMs stay in rocBLAS; these two launches replace MIOpen's many-kernel RNN path and the sampling:
 * pw_bilstm_forward: G [B,N,2,128] = x*W_ih^T + b_ih + b_hh per direction (PyTorch gate order i,f,g,o;
 *   direction 1 = reverse), w_hh_* [128,32] row-major -> H [B,N,64] = [h_forward | h_reverse], ReLU'd
 *   if relu_out (the next layer applies F.relu).  Hidden size is the reference's fixed 32.
 * pw_actor_head: logits [rows,5] = H*W2^T + b2 (optional output) and act[rows] = argmax(logits + g),
 *   g = -log(-log(u)) Gumbel noise from Philox4x32-10 keyed (seed; step, row): the hard one-hot of
 *   F.gumbel_softmax(hard=True) kept as an int32 index on the device. */
/* Y [rows,out_dim] = act(X [rows,in_dim] * W^T + b), W [out_dim,in_dim] row-major, in_dim <= 64, out_dim a
 * multiple of 64, act = ReLU if relu.  ActorNetwork.dense1 + F.relu, and the LSTM input projection
 * x * [W_ih; W_ih_reverse]^T + (b_ih + b_hh) that pw_bilstm_forward consumes. */
int pw_dense(const float *X, const float *W, const float *b, int64_t rows, int32_t in_dim, int32_t out_dim,
             int32_t relu, float *Y, void *stream);
/* G [rows,256] = relu(X [rows,in_dim] * W1^T + b1) * Wih^T + bih in one launch on the matrix cores
 * (v_mfma_f32_32x32x2_f32, exact float32): dense1 + F.relu + the input projections of both LSTM directions.
 * The weights are consumed in MFMA fragment order: pw_actor_front_pack writes that image (w1 [64,in_dim],
 * w_ih [256,64] = [W_ih; W_ih_reverse] row-major -> frag[pw_actor_front_pack_floats(in_dim)]) once per weight
 * update; b_ih [256] = b_ih + b_hh per direction.  in_dim in [1, 104] for pw_actor_front_pack and pw_actor_front
 * (pw_actor_front_kernel<ceil(in_dim / 8)>, 13 instantiations); the image of a given in_dim serves pw_actor_front,
 * pw_actor_fused and pw_policy_rollout alike. */
size_t pw_actor_front_pack_floats(int32_t in_dim);
int pw_actor_front_pack(const float *w1, const float *w_ih, int32_t in_dim, float *frag, void *stream);
int pw_actor_front(const float *X, const float *frag, const float *b1, const float *b_ih, int64_t rows, int32_t in_dim,
                   float *G, void *stream);
int pw_bilstm_forward(const float *G, const float *w_hh_fw, const float *w_hh_bw, int32_t B, int32_t N,
                      int32_t relu_out, float *H, void *stream);
int pw_actor_head(const float *H, const float *w2, const float *b2, int64_t rows, uint64_t seed, uint64_t step,
                  const int64_t *step_dev /* device, or NULL */, float *logits, int32_t *act, void *stream);

/* The whole actor in ONE launch: X [B,N,in_dim] observations -> act (Gumbel-argmax index per head), and/or
 * logits, H [B,N,64] (each optional, NULL to skip).  One head: w2 [n_out0,64], b2 [n_out0], n_out1 = 0,
 * logits [B,N,n_out0], act [B,N].  Two heads (MultiDiscrete actors, main.py:52-54: dense2_1 / dense2_2): w2 / b2 =
 * the two layers concatenated, logits [B,N,n_out0+n_out1] in that order (run.py:39-41), act [B,N,2].
 * n_out0 + n_out1 <= 16.  With n_out0 = 5, n_out1 = 0: same arithmetic and the same Philox keying as
 * pw_actor_front + pw_bilstm_forward + pw_actor_head chained (identical results); G and H stay in LDS.
 * frag = pw_actor_front_pack's image; N <= 96, in_dim in [1, 104].  Kernels: N <= 16 with in_dim <= 64 runs
 * pw_actor_fused16_kernel (16 environments per workgroup), everything else -- N = 17 .. 96, and every in_dim of
 * 65 .. 104 whatever N is -- pw_actor_fused_kernel (min(16, 96 / N) environments per workgroup); same bits. */
int pw_actor_fused(const float *X, const float *frag, const float *b1, const float *b_ih, const float *w_hh_fw,
                   const float *w_hh_bw, const float *w2, const float *b2, int32_t n_out0, int32_t n_out1, int64_t B,
                   int32_t N, int32_t in_dim, int32_t relu_out, uint64_t seed, uint64_t step,
                   const int64_t *step_dev /* device, or NULL */, float *H, float *logits, int32_t *act, void *stream);

/* Optional direct sink of pw_policy_rollout: the chunk's transitions go straight into the replay ring (slot
 * (ring_start + t*B + env) % capacity -- the order of T pw_replay_add calls; next_obs = the PRE-reset observation)
 * and the episode returns are kept in the same launch (episode_return [B] running returns, finished_sum /
 * finished_count accumulated reproducibly; scratch = pw_policy_rollout_scratch_bytes(h) device bytes, zeroed ONCE by the caller and
 * then left to the launches: 0.1.13 -- it is valid for any sequence of launch forms on the handle (pw_set_dispatch policy_form,
 * pw_actor_set_bf16x3 between launches) and for any handle of equal num_envs, one launch at a time; every launch leaves its ticket
 * word zero again.  Word 0 is the ticket, [1, 1 + 2 * workgroups) the partial sums and counts of the last launch).
 * ring may be NULL (bookkeeping only) and episode_return may be NULL (ring only).  0.1.6: the ring may be a STATE ring
 * (pw_replay_store.state_rows) of the handle's scenario (simple_spread with the local observation, simple_tag): the launch then leaves
 * {vel, pos} of every agent before / after the step and the episode's landmarks per transition -- 254 B at C2 instead of 782 -- and
 * pw_replay_gather rebuilds the rows when a batch is sampled (bit-identical to the row ring's batch).  0.1.22: the ring may be a
 * per-agent ring (pw_replay_store.per_agent, rew / done [cap,N]) wherever the form takes a ring: rew[slot, a] is then the value the
 * launch writes to io->rew[t, env, a] and done[slot, a] = 0 (a shared ring: rew[slot] = io->rew_shared[t, env]); slot order, obs,
 * next_obs, act and lm are those of the shared ring, and the episode bookkeeping stays on the shared sum. */
typedef struct pw_rollout_sink {
    const pw_replay_store *ring;
    int64_t ring_start;
    float *episode_return;
    double *finished_sum;
    int64_t *finished_count;
    void *scratch;
} pw_rollout_sink;

/* Policy-in-the-loop rollout as ONE launch: num_steps x (actor forward + Gumbel sampling + environment step +
 * auto-reset) on the handle's bound state, starting from the observation of the current state; observations,
 * sampled actions and world state stay on the CU between steps.  io: the pw_rollout outputs ([num_steps, ...];
 * no action inputs, no coll); act_out [num_steps,B,N] int32 receives the sampled indices.  Without a sink (sink NULL,
 * or one with neither a ring nor episode_return) act_out and obs, rew, rew_shared, done, terminal are required (final_obs
 * optional); with one -- a ring, the episode bookkeeping or both -- every output is optional, each on its own: what is
 * left out changes no other output, no ring slot, no statistic and not the state the launch leaves
 * (tests/test_gpu_rollout_output_subsets.py).  The Gumbel noise of step t is keyed (seed; step + t, row) exactly as pw_actor_fused / pw_actor_head, so
 * the results equal a loop of pw_actor_fused + pw_step (+ pw_replay_add_tail).
 * simple_spread fast-path configurations (local observation, homogeneous agents, L <= N; observation rows up to
 * D = 104, i.e. N = L <= 50: rows longer than 64 numbers on the just-in-time kernel form only) and simple_tag with homogeneous roles (9 <= D <= 48; good agents' rows zero-padded to D), one
 * 5-logit head; weights as for pw_actor_fused.
 * simple_reference (the MultiDiscrete scenario of main.py:24,52-54; 3 landmarks, D = 21): the two-head actor -- w2 [5 + PW_DIM_C,
 * 64] / b2 = dense2_1 and dense2_2 concatenated, one Gumbel-argmax per head exactly as pw_actor_fused(n_out0 = 5, n_out1 =
 * PW_DIM_C) -- and act_out [num_steps,B,N,2] = (movement, symbol); the ring sink must be the two-head ring (act_heads = 2, head widths
 * 5 | PW_DIM_C, shared-reward or per-agent; 0.1.5 -- before, the chunk went into it with a second launch, pw_replay_add_rollout); results equal a loop of
 * pw_actor_fused + pw_step(act_idx, act_comm).
 * Every other simple_spread / simple_tag configuration pw_step serves (0.1.9: the full observation, L > N, landmark contact on
 * simple_spread, per-agent sizes / accelerations / speed clamps, a simple_tag roster with one agent unlike its role, a handle with
 * pw_dispatch.force_generic): the generic form, pw_policy_rollout_generic_kernel -- the arithmetic of pw_rollout_kernel, so the same
 * bits as the pw_actor_fused + pw_step loop; one 5-logit head, exact float32 only, rows of at most 64 numbers, at most 96 rows and
 * 160 KB of LDS per workgroup (pw_policy_generic_envs_per_workgroup; PW_EINVAL naming N and D otherwise); the sink takes the single-head
 * row ring only, shared-reward or per-agent (a STATE or two-head ring is PW_EINVAL).  Selected automatically for the handles the forms above refuse
 * -- except handles whose agents differ within a role (size, acceleration, force scale or speed clamp unlike the role's first
 * agent), which stay PW_EINVAL under automatic dispatch -- and on any simple_spread / simple_tag handle by pw_dispatch.policy_form = 5. */
int pw_policy_rollout(pw_handle *h, const float *frag, const float *b1, const float *b_ih, const float *w_hh_fw,
                      const float *w_hh_bw, const float *w2, const float *b2, int32_t relu_out, uint64_t seed,
                      uint64_t step, const int64_t *step_dev /* device, or NULL */, const pw_step_io *io,
                      int32_t *act_out, int32_t num_steps, const pw_rollout_sink *sink /* or NULL */, void *stream);
size_t pw_policy_rollout_scratch_bytes(const pw_handle *h);
/* Environments per 512-thread workgroup of the generic form for a configuration (host arithmetic only, no device): the largest
 * E <= 16 with E * N <= 96 rows whose LDS layout fits 160 KB, or 0 when none does or the observation row is longer than 64 numbers
 * (pw_policy_rollout then returns PW_EINVAL).  obs_mode applies to simple_spread, A (adversaries) to simple_tag. */
int pw_policy_generic_envs_per_workgroup(int32_t scenario, int32_t obs_mode, int32_t N, int32_t L, int32_t A);

/* Test hook: y[i] = f(x[i]) with the DEVICE implementation of one math primitive, so its bits can be compared
 * with a CPU implementation of pworld_math.h.  fn: 0 the kernels' fast correctly-rounded sqrt, 1 their
 * branch-free softplus, 2 pw_softplus, 3 pw_exp, 4 sqrtf, 5 x / aux (IEEE division), 6 / 7 the hot loops'
 * scaling-free division chain for x / aux and aux / x, 8 their softplus, 9 aux / x (IEEE division), 10 x / aux with ONE
 * correction step (what the C2 kernel runs for the division by the contact margin when pw_margin_one_correction(aux)),
 * 11 / 12 the hot loops' correctly rounded sqrt for x in [2^-90, 2^90) (one fused correction) / the two-test form it replaced. */
int pw_debug_math(int32_t fn, const float *x, float aux, float *y, int64_t n, void *stream);
/* 1 if dividing by this contact margin with one Newton correction is IEEE division (its refined reciprocal is the correctly
 * rounded one, from every 1-ulp-accurate starting value; significand not all ones; inside the division chain's range): the
 * host-side decision behind the K1 kernel instantiations.  The canonical margin 1e-3 qualifies. */
int pw_margin_one_correction(float contact_margin);

/* The learner's critic (rls/model/ac_network_multi_gumbel.py CriticNetwork) and, optionally, the TD target of
 * ddpg_gumbel_fix.py:148-154 as ONE launch: q [b] = dense2(relu(attention(LSTM(relu(dense1([obs | action])))))) in float32 --
 * one-layer LSTM (hidden 64, gates i, f, g, o, zero initial state) over the agent axis, score_t = <out_t, h_N>, softmax over t,
 * weighted sum.  obs [b,N,obs_dim].  Action, exactly one of: act_idx int32 [b,N] (n_act1 = 0) or [b,N,2] (two heads, widths
 * n_act0 | n_act1; an index outside its head selects no column) or act_vec float [b,N,n_act0 + n_act1].  An exact one-hot
 * act_vec and the equal indices give the same bits.  Weights in nn.Module layout: w1 [64, obs_dim + A] / b1 = dense1.module,
 * w_ih / w_hh [256,64], b_ih / b_hh [256] = lstm.*_l0, w2 [1,64] / b2 [1] = dense2.  With rew [b], done [b] (float) and y [b]
 * (all three or none): y = rew + gamma * q * (1 - done), evaluated left to right without contraction on the q this launch
 * writes.  N in [1, 64], obs_dim in [1, 104], n_act0 + n_act1 <= 16, any b >= 1.  All pointers are device memory. */
int pw_critic_forward(const float *obs, const int32_t *act_idx, const float *act_vec, int32_t n_act0, int32_t n_act1,
                      const float *w1, const float *b1, const float *w_ih, const float *w_hh, const float *b_ih,
                      const float *b_hh, const float *w2, const float *b2, int64_t b, int32_t N, int32_t obs_dim,
                      const float *rew /* or NULL */, const float *done /* or NULL */, float gamma, float *q,
                      float *y /* or NULL */, void *stream);

/* The BiCNet baseline's critic (rls/model/ac_network_multi_gumbel_BIC.py CriticNetwork) and, optionally, the per-agent TD target of
 * BIC_gumbel_fix.py:155-160 as ONE launch: q [b,N], q[r][t] = <w2, h_t[r]> + b2 on the LSTM's output of step t itself (no ReLU, no
 * attention) -- front end, recurrence, action forms, weight layout (w2 [1,64] / b2 [1] = dense2.module) and every limit as
 * pw_critic_forward.  With rew [b,N], done [b,N] (float) and y [b,N] (all three or none): y = rew + gamma * q * (1 - done) element-wise,
 * left to right without contraction.  q[r][t] depends on agents 0 .. t of row r only (not on N). */
int pw_critic_forward_steps(const float *obs, const int32_t *act_idx, const float *act_vec, int32_t n_act0, int32_t n_act1,
                            const float *w1, const float *b1, const float *w_ih, const float *w_hh, const float *b_ih,
                            const float *b_hh, const float *w2, const float *b2, int64_t b, int32_t N, int32_t obs_dim,
                            const float *rew /* [b,N] or NULL */, const float *done /* [b,N] or NULL */, float gamma,
                            float *q /* [b,N] */, float *y /* [b,N] or NULL */, void *stream);

/* The model-learning variant's critic (rls/model/ac_network_model_multi_gumbel.py CriticNetwork) and, optionally, the TD target of
 * model_ddpg_gumbel_fix.py:158-163 as ONE launch: the attention critic of pw_critic_forward WITHOUT the ReLU on the context and with
 * two heads on it, q [b] = <w2, ctx> + b2 and r_pred [b] = <w3, ctx> + b3 (w3 [1,64] / b3 [1] = dense3), both summed in one order:
 * equal heads give equal bits.  r_pred == NULL stores no reward prediction, and then w3 / b3 may be NULL (the target critic); r_pred
 * without w3 / b3 is PW_EINVAL.  y as in pw_critic_forward, from this launch's q.  Action forms, weight layout and every limit as
 * pw_critic_forward. */
int pw_critic_forward_model(const float *obs, const int32_t *act_idx, const float *act_vec, int32_t n_act0, int32_t n_act1,
                            const float *w1, const float *b1, const float *w_ih, const float *w_hh, const float *b_ih,
                            const float *b_hh, const float *w2, const float *b2, const float *w3 /* or NULL */,
                            const float *b3 /* or NULL */, int64_t b, int32_t N, int32_t obs_dim, const float *rew /* or NULL */,
                            const float *done /* or NULL */, float gamma, float *q, float *r_pred /* or NULL */,
                            float *y /* or NULL */, void *stream);

/* The tail of a network's update as ONE launch (csrc/pw_kernels_optim.hpp states the float32 operation order):
 *   total_norm = sqrt(sum g^2) over ALL tensors of the call; coef = min(1, max_norm / (total_norm + 1e-6))   [torch.nn.utils.clip_grad_norm_]
 *   g = grad * coef; g += weight_decay * p; Adam (torch.optim.Adam without amsgrad / maximize) on exp_avg, exp_avg_sq, param, in place;
 *   target = target * (1 - tau) + param * tau on the NEW param, where target != NULL                         [ddpg_gumbel_fix.py:36-47]
 * `step` is the step this call takes (>= 1); the bias corrections are formed from it in float64 on the host.  Hyper-parameters are
 * doubles, as torch holds them: 1 - beta1, 1 - beta2 and 1 - tau are formed in float64 and rounded to float32 once.
 * Gradients are READ, never written (clip_grad_norm_ scales .grad in place; here the scaled gradient lives in registers).
 * A NaN gradient makes total_norm and coef NaN and so every element of a clipping call, as clip_grad_norm_ does.
 * The norm is summed in a fixed order without atomics: the same inputs give the same bits, every element of a call sees the
 * same coef, and no workgroup waits for another.  total_norm (device, may be NULL) receives the norm, also with max_norm <= 0.
 * The table travels in the kernel arguments: no copy, no allocation, no synchronisation; one launch on `stream`.
 * Tensors: device float32, any 4-byte aligned address, any numel >= 1; at most PW_OPT_MAX_TENSORS tensors and 2^20 elements
 * per call.  PW_EINVAL (nothing launched): count outside [1, 32], more than 2^20 elements, a null param / grad / exp_avg /
 * exp_avg_sq, numel < 1, step < 1, lr < 0, beta outside [0, 1), eps < 0, weight_decay < 0, tau outside [0, 1] with a target. */
#define PW_OPT_MAX_TENSORS 32
typedef struct pw_opt_tensor {
    float *param;
    const float *grad;
    float *exp_avg;
    float *exp_avg_sq;
    float *target; /* may be NULL: no soft update for this tensor */
    int64_t numel;
} pw_opt_tensor;
int pw_adam_step(const pw_opt_tensor *tensors, int32_t count, int64_t step, double lr, double beta1, double beta2, double eps,
                 double weight_decay, double max_norm /* <= 0: no clipping */, double tau /* used where target != NULL */,
                 float *total_norm /* device, or NULL */, void *stream);
/* pw_adam_step with the step count in device memory (a captured launch freezes by-value arguments): *step_dev (8-byte aligned) is
 * the step this call takes, a value below 1 counts as 1; advance it with pw_counter_add(step_dev, 1, 0, stream).  Same table,
 * hyper-parameters, limits and arithmetic; the kernel forms the two step-dependent scalars itself, in float64:
 *   bc2_sqrt = (float)sqrt(1 - beta2^t), step_size = (float)(lr / (1 - beta1^t)), beta^t by square-and-multiply, least significant
 *   bit first (r = 1; x = beta; while t: if t & 1: r *= x; x *= x; t >>= 1) -- multiplications only, so host and device agree bit
 * for bit (csrc/pw_optim_bias.hpp).  pw_adam_step uses std::pow; after rounding to float32 the two forms agree at every t <= 20000
 * for (beta1, beta2, lr) in {(0.9, 0.999, 1e-2), (0.9, 0.999, 1e-3), (0.8, 0.99, 3e-4)}.  PW_EINVAL as pw_adam_step, and a null or
 * misaligned step_dev. */
int pw_adam_step_dev(const pw_opt_tensor *tensors, int32_t count, const int64_t *step_dev, double lr, double beta1, double beta2,
                     double eps, double weight_decay, double max_norm, double tau, float *total_norm, void *stream);
/* out[0] = bc2_sqrt, out[1] = step_size of pw_adam_step_dev at `step`, formed on the host by the same function. */
void pw_adam_bias_scalars(int64_t step, double lr, double beta1, double beta2, float out[2]);
/* target[k] = target[k] * (1 - tau) + source[k] * tau for count tensor pairs of numel[k] elements, one launch: both products
 * rounded to float32 before the sum, bit for bit torch's `t * (1.0 - tau) + s * tau`.  tau == 1 copies (an infinity in the old
 * target does not become NaN).  The three arrays are HOST arrays of device pointers / sizes; limits as pw_adam_step. */
int pw_soft_update(float *const *target, const float *const *source, const int64_t *numel, int32_t count, double tau, void *stream);

/* The recurrent part of a one-layer LSTM WITH gradient (csrc/pw_kernels_lstm.hpp), one launch each, for the learner's three passes per
 * update.  Gate order i, f, g, o as in PyTorch.  Shapes served: dirs = 1, H = 64 (CriticNetwork.lstm, BiCNetCritic.lstm) and dirs = 2,
 * H = 32 (ActorNetwork.bilstm; direction 1 walks t = N - 1 .. 0); b >= 1 and N >= 1 arbitrary.  Everything else, a null or
 * misaligned pointer, w_hh_bw null with dirs = 2 or set with dirs = 1: PW_EINVAL naming the argument, nothing launched.
 * G [b,N,dirs,4H] = x W_ih^T + b_ih + b_hh (the caller's GEMM), w_hh_* [4H,H] as nn.LSTM keeps them
 * (views into the flat buffer: any 4-byte aligned address), w_hh_bw NULL when dirs = 1.
 * Y [b,N,dirs*H] = [h_forward | h_reverse].  saved: NULL (no gradient wanted: nothing is stored) or
 * [b,N,dirs,5,H] = i, f, g, o (after activation) and c of every step.  Initial h and c are zero.  The saved gates are formed for the
 * backward (accurate in 1 - gate where a gate saturates: csrc/pw_kernels_lstm.hpp) and may differ in the last bits from those behind Y.
 * Activations are pw_lstm_math.hpp's (v_exp_f32 / v_rcp_f32): results differ from MIOpen's in the last bits.  No atomics, fixed
 * summation order: the same inputs give the same bits. */
int pw_lstm_train_forward(const float *G, const float *w_hh_fw, const float *w_hh_bw, int64_t b, int32_t N,
                          int32_t dirs, int32_t H, float *Y, float *saved, void *stream);
/* dY [b,N,dirs*H] contiguous -> dG [b,N,dirs,4H]: the gradient at the pre-activations.  The recurrent part only: per sequence and
 * direction the steps in the reverse of their forward order, from dh = dc = 0, with c_prev the forward order's previous c and
 * tc = tanh(c_t) recomputed with the forward's function:
 *   dh_t = dY_t + dh;  do = dh_t tc o(1-o);  dc_t = dc + dh_t o (1-tc^2);  di = dc_t g i(1-i);  df = dc_t c_prev f(1-f);
 *   dg = dc_t i (1-g^2);  dG_t = [di, df, dg, do];  dh = dG_t . W_hh;  dc = dc_t f.
 * The gradients of W_ih, the biases and x are GEMMs and the caller's (multiagent_rl_amd/lstm.py); those of W_hh (dG^T against the
 * shifted Y) are the caller's GEMMs too, or pw_lstm_train_wgrad below. */
int pw_lstm_train_backward(const float *dY, const float *saved, const float *w_hh_fw, const float *w_hh_bw, int64_t b,
                           int32_t N, int32_t dirs, int32_t H, float *dG, void *stream);
/* The two recurrent-weight gradients (csrc/pw_kernels_lstm_wgrad.hpp, translation unit pworld_lstm_wgrad.hip), from dG [b,N,dirs,4H] as pw_lstm_train_backward writes it and Y [b,N,dirs*H] as
 * pw_lstm_train_forward writes it, both read in place (no shifted copy exists in memory):
 *   dw_hh_fw[r][k] = sum over seq and t = 1 .. N-1 of dG[seq][t][0][r] * Y[seq][t-1][k]
 *   dw_hh_bw[r][k] = sum over seq and t = 0 .. N-2 of dG[seq][t][1][r] * Y[seq][t+1][H+k]          r < 4H, k < H
 * Both [4H,H], any 4-byte aligned address.  Either may be NULL: that direction is skipped (not multiplied, not written).  With
 * N = 1 the sums are empty and the outputs are written as exact zeros.  Exact float32 on v_mfma_f32_16x16x4_f32; TWO launches for
 * both directions together: one forms a partial sum per workgroup (at most 128; rows (seq, t) ascending in tiles of 16, two
 * accumulator chains per output) in `scratch`, the other adds the partial sums as a balanced tree over the workgroup numbers.  No
 * floating-point atomics: the order of every sum is a function of (b, N, dirs) alone, so the same inputs give the same bits on every
 * launch, on every stream, eager or replayed from a graph.  A row without a previous step in its direction (t = 0 forward, t = N-1
 * reverse) contributes nothing BY A SELECT, not by a product with zero: a NaN in dG[:, 0, 0] or dG[:, N-1, 1] does not reach the
 * outputs, as it does not reach the sliced GEMMs these sums replace; the shifted row never comes from the neighbouring sequence.
 * scratch: pw_lstm_train_wgrad_scratch_bytes(b, N, dirs, H) bytes of device memory, 4-byte aligned, contents arbitrary; it belongs to
 * the call until its launches have run (0 from that function = the shape is not served).
 * PW_EINVAL, nothing launched: a shape other than dirs = 1, H = 64 / dirs = 2, H = 32, b < 1, N < 1, b N > 2^40, dG / Y / scratch
 * null, both outputs null, dw_hh_bw set with dirs = 1, a misaligned pointer. */
size_t pw_lstm_train_wgrad_scratch_bytes(int64_t b, int32_t N, int32_t dirs, int32_t H);
int pw_lstm_train_wgrad(const float *dG, const float *Y, int64_t b, int32_t N, int32_t dirs, int32_t H, float *dw_hh_fw,
                        float *dw_hh_bw, void *scratch, void *stream);

/* The attention block of CriticNetwork WITH gradient (csrc/pw_kernels_attention.hpp), one launch each, for the learner's two critic
 * passes per update.  Y [b,N,H] is the LSTM's output; the query is its last step, q = Y[:, N-1] (h_n[-1] of a one-direction LSTM).
 *   s_t = <Y_t, q>;  w = softmax_t(s) (maximum subtracted, expf as in pw_critic_forward);  c = sum_t w_t Y_t, t ascending;
 *   out [b,H] = relu ? max(c, 0) : c;  weight [b,N] = w, or NULL: nothing is stored (no gradient wanted).
 * Served: H = 64, 1 <= N <= 64 (pw_critic_forward's agent-axis bound), b >= 1.  Everything else, a null required pointer or a
 * pointer that is not 4-byte aligned (all loads and stores are 4 bytes wide): PW_EINVAL naming the argument, nothing launched.
 * No atomics, fixed summation order: the same inputs give the same bits, with and without weight, on any stream. */
int pw_attention_pool_forward(const float *Y, int64_t b, int32_t N, int32_t H, int32_t relu, float *out, float *weight, void *stream);
/* dOut [b,H] contiguous, Y, weight and out as the forward read and wrote them -> dY [b,N,H]:
 *   dc = relu ? dOut [out > 0] : dOut;  dw_t = <Y_t, dc>;  ds_t = w_t (dw_t - sum_u w_u dw_u);  dY_t = w_t dc + ds_t q;
 *   dY_{N-1} += dq = sum_t ds_t Y_t (t ascending): the last step receives its score's gradient as a step and as the query. */
int pw_attention_pool_backward(const float *dOut, const float *Y, const float *weight, const float *out, int64_t b, int32_t N,
                               int32_t H, int32_t relu, float *dY, void *stream);

/* The learner's Gumbel-softmax sample WITH gradient (csrc/pw_kernels_sample.hpp), one launch each: F.gumbel_softmax(logits, tau, hard)
 * on logits [rows,n] float32, 1 <= n <= 16, tau > 0, with the library's own noise instead of torch's generator.
 *   step_eff = step + (step_dev ? *step_dev : 0)   (step_dev: an int64 device cell, read by the kernel -- a replayed launch of a
 *     captured graph draws new noise when the cell has been advanced, e.g. by pw_counter_add);
 *   noise(r, o) = log(-log u), u from word (o & 3) of Philox4x32-10 block (o >> 2), counter (r lo, r hi | tag(blk), step_eff lo,
 *     step_eff hi), key seed, tag(blk) = ((blk & 1) << 31) | ((blk >> 1) << 30): the draw of the actor heads (pw_actor_head), so a
 *     learner must use another seed than its exploration actor;
 *   v = (logit - noise) / tau;  idx = the first maximum of v;  soft = softmax(v), maximum subtracted, summed o ascending;
 *   y [rows,n] = hard ? (onehot(idx) - soft) + soft : soft   (the VALUE of torch's y_hard - y_soft.detach() + y_soft).
 * soft [rows,n] (what the backward needs), idx [rows] int32 and noise [rows,n] (the values subtracted) are optional: NULL stores
 * nothing.  A bad n / tau / rows, a null logits or y, a misaligned pointer: PW_EINVAL naming the argument, nothing launched.
 * One thread per row, no atomics: the same (inputs, seed, step_eff) give the same bits on any stream. */
int pw_gumbel_st_forward(const float *logits, int64_t rows, int32_t n, float tau, int32_t hard, uint64_t seed, uint64_t step,
                         const int64_t *step_dev, float *y, float *soft, int32_t *idx, float *noise, void *stream);
/* dY [rows,n] contiguous and soft as the forward wrote it -> dLogits [rows,n]:
 *   dLogits_o = soft_o (dY_o - sum_k dY_k soft_k) / tau, k ascending -- the soft sample's gradient, which the hard sample shares. */
int pw_gumbel_st_backward(const float *dY, const float *soft, int64_t rows, int32_t n, float tau, float *dLogits, void *stream);

/* ---- the dense front of the learner's networks with gradient (translation unit pworld_front.hip) -----------------------------------
 * [x0 | x1] -> dense1 (w1 [64, d0 + d1], b1 [64]) -> ReLU -> G = hid W_ih^T + (b_ih + b_hh), exact float32:
 *   x0 [rows,d0], x1 [rows,d1] or NULL with d1 = 0: the two parts of the input row, read side by side (no concatenated copy);
 *   per direction d < dirs: w_ih[d] [4H,64], b_ih[d], b_hh[d] [4H] as nn.LSTM keeps them, read in place (with dirs = 1 entry 1 is unread);
 *   hid [rows,64] after the ReLU, or NULL when no gradient will need it; G [rows, dirs*4H] as pw_lstm_train_forward reads it.
 * Served: (dirs, H) = (1, 64) or (2, 32), 1 <= d0 <= 104, 0 <= d1 <= 16, rows >= 1; anything else, a null argument, an input that is not
 * 4-byte aligned or a hid / G that is not 16-byte aligned: PW_EINVAL naming it, nothing launched.  One launch. */
int pw_front_train_forward(const float *x0, int32_t d0, const float *x1, int32_t d1, const float *w1, const float *b1,
                           const float *const w_ih[2], const float *const b_ih[2], const float *const b_hh[2], int64_t rows,
                           int32_t dirs, int32_t H, float *hid, float *G, void *stream);
/* dG [rows, dirs*4H] contiguous, the forward's inputs and its hid ->
 *   dHid = (dG W_ih) o (hid > 0);  dW_ih[d] = dG_d^T hid;  db_gate[d] = sum over rows of dG_d (one vector serves b_ih and b_hh);
 *   dW1 = dHid^T [x0 | x1];  db1 = sum over rows of dHid;  dx0 / dx1 = dHid W1 split by column, each only when its pointer is given.
 * Two launches: the main kernel leaves one partial sum per workgroup and element in `scratch` (at least
 * pw_front_train_scratch_bytes(rows, d0, d1) bytes), the second adds them in workgroup order.  The number of workgroups and the rows of
 * each follow from `rows` alone and no floating-point atomic exists: the same inputs give the same bits on every launch. */
int pw_front_train_backward(const float *dG, const float *x0, int32_t d0, const float *x1, int32_t d1, const float *hid,
                            const float *w1, const float *const w_ih[2], int64_t rows, int32_t dirs, int32_t H, float *dW1, float *db1,
                            float *const dW_ih[2], float *const db_gate[2], float *dx0, float *dx1, void *scratch,
                            size_t scratch_bytes, void *stream);
/* The bytes of scratch one pw_front_train_backward of this shape needs (0 for a shape that is not served). */
size_t pw_front_train_scratch_bytes(int64_t rows, int32_t d0, int32_t d1);

/* ---- the output layers of the learner's networks with gradient (translation unit pworld_head.hip) -----------------------------------
 * A = relu ? max(X, 0) : X (a NaN stays one);  out_k = A W_k^T + b_k for k < heads, exact float32:
 *   X [rows,64]; w[k] [n[k],64], b[k] [n[k]] as nn.Linear keeps them, read in place; out[k] [rows,n[k]]; w, b, n and out hold `heads` entries.
 * Served: 1 <= heads <= 3, 1 <= n[k] <= 104, rows >= 1; anything else, a null argument or a pointer that is not 4-byte aligned:
 * PW_EINVAL naming it, nothing launched.  One launch for all heads; X is read once and A is never stored. */
int pw_head_train_forward(const float *X, int64_t rows, int32_t relu, int32_t heads, const float *const *w, const float *const *b,
                          const int32_t *n, float *const *out, void *stream);
/* dOut[k] [rows,n[k]] contiguous, or NULL for a head that received no gradient, and the forward's X ->
 *   dX [rows,64] = (sum over the heads with a dOut of dOut_k W_k) o (relu ? X > 0 : 1), or nothing when dX is NULL;
 *   dW[k] [n[k],64] = dOut_k^T A;  db[k] [n[k]] = sum over rows of dOut_k   for every head with a dOut.
 * A head whose dOut is NULL adds nothing to dX, its dW[k] and db[k] must be NULL too and nothing is computed for it; a launch in which
 * only head 0 has a dOut gives the bits of the one-head launch.  Every dOut NULL, a dW or db beside a NULL dOut, a missing dW or db
 * beside a dOut, a dX that is not 16-byte aligned, any other pointer that is not 4-byte aligned: PW_EINVAL, nothing launched.
 * Two launches: the main kernel leaves one partial sum per workgroup and element in `scratch` (at least
 * pw_head_train_scratch_bytes(rows, heads, n) bytes), the second adds them as a balanced tree over the workgroups (db, and that tree, as
 * compensated sums: a bias gradient that nearly cancels keeps one rounding of its result, not of its partial sums); with rows <= 16 one
 * workgroup holds every row and the main kernel stores the results itself (one launch).  The number of workgroups and the rows of
 * each follow from `rows` alone and no floating-point atomic exists: the same inputs give the same bits on every launch. */
int pw_head_train_backward(const float *const *dOut, const float *X, int64_t rows, int32_t relu, int32_t heads, const float *const *w,
                           const int32_t *n, float *dX, float *const *dW, float *const *db, void *scratch, size_t scratch_bytes,
                           void *stream);
/* The bytes of scratch one pw_head_train_backward of this shape needs, whichever of its heads have a dOut (0 for a shape that is not
 * served). */
size_t pw_head_train_scratch_bytes(int64_t rows, int32_t heads, const int32_t *n);

/* ---- the episode log: per-episode, per-agent returns of a chunk (translation unit pworld_episode_log.hip) ------------------------------
 * One launch sequence consumes the planes of one chunk, whoever produced them (pw_rollout, pw_policy_rollout, a step loop, the side
 * buffers of a gather): rew [T,B,N] float32 and terminal [T,B] uint8, and appends one entry per finished episode to a log the caller
 * owns (experiments/run.py:55-65, for B worlds stepped side by side).  All arrays, the two cells and the scratch are device memory.
 *   Arithmetic: float64 accumulators, float32 rewards widened.  Per step, for env e: by_agent[a] += rew[t,e,a] for every agent, and
 *   total += rew[t,e,0], then ... + rew[t,e,N-1], agents ascending -- total is a sum of its own, not the sum of the shares.  Where
 *   terminal[t,e] is set the entry is stored and the env's carry becomes +0.0 by assignment: a NaN or Inf reward poisons the sums of
 *   its own episode and nothing else.  No floating-point atomic: the results are a function of the inputs alone, bit for bit.
 *   Order: entry k of a launch goes to slot *length + k, k = the number of set flags before (t, e) in row-major order of terminal
 *   (by end step, then by env).
 *   Capacity: an entry whose slot is >= capacity is not stored (nothing is written past the arrays); *length and carry advance as if it
 *   had been: the caller sees *length > capacity.
 *   Cells: *length += the chunk's finished episodes, *step_base += T, from the launch itself: no host value changes per chunk.
 * PW_EINVAL, nothing launched: a wrong struct_size, a null pointer, a total / by_agent / end_step / carry / length / step_base that is
 * not 8-byte aligned, an env or rew that is not 4-byte aligned, a scratch that is not 16-byte aligned, capacity < 1, T < 1, num_envs < 1,
 * num_agents outside 1 .. PW_EPISODE_LOG_MAX_AGENTS, T * num_envs > 2^31 - 1 (the slot plane holds int32), num_envs * (num_agents + 1) >= 2^32
 * (the walk's grid).  PW_EHIP (a launch the runtime refused): the cells may already have advanced; the log is invalid, discard it. */
#define PW_EPISODE_LOG_MAX_AGENTS 96
typedef struct pw_episode_log {
    uint32_t struct_size;      /* = sizeof(pw_episode_log); checked */
    int32_t  num_envs, num_agents;
    int64_t  capacity;         /* entries */
    double  *total;            /* [capacity]     return of the episode over all agents */
    double  *by_agent;         /* [capacity, N]  each agent's share */
    int64_t *end_step;         /* [capacity]     batched step index at which it ended (*step_base + t) */
    int32_t *env;              /* [capacity]     env index within this handle / rank */
    double  *carry;            /* [B, N + 1]     returns of the episodes in progress, column N = total; zeroed once by the caller */
    int64_t *length;           /* device cell: episodes finished so far (keeps counting past capacity) */
    int64_t *step_base;        /* device cell: batched steps absorbed so far; the launch adds T */
    void    *scratch;          /* pw_episode_log_scratch_bytes(T, B) bytes; contents need not survive between launches */
} pw_episode_log;
/* The bytes of scratch one pw_episode_log_absorb of T steps over B envs needs (0 for a shape that is not served). */
size_t pw_episode_log_scratch_bytes(int32_t T, int32_t B);
int pw_episode_log_absorb(const pw_episode_log *log, const float *rew, const uint8_t *terminal, int32_t T, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PWORLD_H */
