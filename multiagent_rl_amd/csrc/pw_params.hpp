// pw_params.hpp -- part of libpworld.so: the kernel parameter blocks that the handle keeps and the host fills in (passed by
// value in the kernarg segment).  The kernels that read them are in pw_kernels_generic.hpp (KParams), pw_kernels_spread.hpp
// (FastConsts, StreamParams), pw_kernels_tag.hpp (TagParams) and pw_kernels_reference.hpp (RefParams).
#pragma once

#include "pworld.h"

namespace {

// Everything a kernel needs, passed by value in the kernarg segment.
struct KParams {
    int B, N, L, A, D;
    int epw;          // envs per wave
    int max_episode_len, auto_reset, force_discrete, landmark_collide;
    uint64_t seed, env_id_base;
    float dt, damp, contact_force, contact_margin, mass, landmark_size;
    float *pos_x, *pos_y, *vel_x, *vel_y, *lm_x, *lm_y;
    int32_t *ep_step;
    uint32_t *ep_count;
    float agent_size[PW_MAX_AGENTS];
    float agent_sens[PW_MAX_AGENTS];      // accel if set else default_sensitivity (_set_action)
    float agent_fscale[PW_MAX_AGENTS];    // 1, or mass*accel with the fork knob (apply_action_force)
    float agent_max_speed[PW_MAX_AGENTS]; // < 0: None
};

// simple_spread fast path: the constants derived on the host (pworld.hip setup_fast_path)
struct FastConsts {
    float dist_min, coll_thr2, near_thr2, sens, fscale, size;
    int k1;  // the contact margin qualifies for the one-correction division (margin_one_correction)
};

// simple_spread streaming / duo / quad kernels
struct StreamParams {
    int B, N, L, epw, max_episode_len, auto_reset;
    int p_prio;  // duo kernel: issue priority per wave, 2 bits each (wave 0 = physics in bits 0-1, ...); set by the launch
    uint64_t seed, env_id_base;
    float dt, damp, contact_force, contact_margin, mass;
    float dist_min, coll_thr2, near_thr2, sens, fscale;
    float *pos_x, *pos_y, *vel_x, *vel_y, *lm_x, *lm_y;
    int32_t *ep_step;
    uint32_t *ep_count;
    const int32_t *act;
    float *obs, *final_obs, *rew, *rew_shared;
    uint8_t *done, *terminal;
    uint64_t *coll;  // [T,B,N] collision masks; written only by the COLL instantiations
};

// simple_tag streaming / duo kernels
struct TagParams {
    int B, N, L, A, D, epw, max_episode_len, auto_reset;
    int p_prio;     // duo kernel: raise the physics wave's issue priority (set by the launch: small and mid-size grids)
    int obs_block;  // duo kernel: stage the wave's observation rows in LDS and store them as one contiguous block (0 / 2 / 4 = chunk floats)
    uint64_t seed, env_id_base;
    float dt, damp, contact_force, contact_margin, mass;
    float sens[2], fscale[2], max_speed[2];
    float dist_min[2][2], coll_thr2[2][2], near_thr2[2][2];  // [class_i][class_j]
    float dist_min_lm[2], near_thr2_lm[2];                   // agent class vs landmark
    float *pos_x, *pos_y, *vel_x, *vel_y, *lm_x, *lm_y;
    int32_t *ep_step;
    uint32_t *ep_count;
    const int32_t *act;
    float *obs, *final_obs, *rew, *rew_shared;
    uint8_t *done, *terminal;
    uint64_t *coll;  // [T,B,N] collision masks; written only by the COLL instantiations
};

// the communication scenarios (simple_reference, simple_speaker_listener)
struct RefParams {
    int B, L, D, max_episode_len, auto_reset, force_discrete;
    uint64_t seed, env_id_base;
    float dt, damp, mass, sens;
    float *pos_x, *pos_y, *vel_x, *vel_y, *lm_x, *lm_y, *comm;
    int32_t *goal, *ep_step;
    uint32_t *ep_count;
};

}  // namespace
