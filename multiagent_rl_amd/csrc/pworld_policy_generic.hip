// libpworld.so, sixth translation unit -- the one-launch policy rollout of the configurations only the generic environment kernel
// serves (pw_kernels_policy_generic.hpp): its shape search and its launcher.  pw_policy_rollout (pworld_policy.hip) hands the call over
// (pw_dispatch.policy_form = 5, or automatically where forms 3 / 3j / tag do not apply).  A unit of its own: the policy unit's build
// time and code object stay as they are.
#include "pw_handle.hpp"
#include "pw_policy_host.hpp"
#include "pw_kernels_policy_generic.hpp"

namespace {

// observation length of a simple_spread / simple_tag configuration (pworld.hip obs_dim_of), -1 for anything else
int generic_obs_dim(int scenario, int obs_mode, int N, int L, int A)
{
    if (scenario == PW_SIMPLE_SPREAD) return obs_mode == PW_OBS_FULL ? 4 + 2 * L + 4 * (N - 1) : 4 + 2 * L;
    if (scenario == PW_SIMPLE_TAG) return 4 + 2 * L + 2 * (N - 1) + 2 * (A > 0 ? N - A : N - A - 1);   // the widest row: an adversary's
    return -1;
}

}  // namespace

extern "C" {

int pw_policy_generic_envs_per_workgroup(int32_t scenario, int32_t obs_mode, int32_t N, int32_t L, int32_t A)
{
    if (N < 1 || N > PW_MAX_AGENTS || L < 0 || L > PW_MAX_LANDMARKS || A < 0 || A > N) return 0;
    if (obs_mode != PW_OBS_LOCAL && obs_mode != PW_OBS_FULL) return 0;
    const int D = generic_obs_dim(scenario, obs_mode, N, L, A);
    if (D < 1 || D > 64) return 0;
    const int S1 = 4 * ((D + 7) / 8);
    for (int e = kFusedRows / N < 16 ? kFusedRows / N : 16; e >= 1; --e)
        if (policy_generic_lds(S1, D, e, N, L).bytes <= 160 * 1024) return e;
    return 0;
}

__attribute__((visibility("hidden")))
int pw_internal_policy_rollout_generic(pw_handle *h, const float *frag, const float *b1, const float *b_ih, const float *w_hh_fw,
                                       const float *w_hh_bw, const float *w2, const float *b2, int32_t relu_out, uint64_t seed,
                                       uint64_t step, const int64_t *step_dev, const pw_step_io *io, int32_t *act_out,
                                       int32_t num_steps, const pw_rollout_sink *sink, void *stream)
{
    const KParams &kp = h->kp;
    const int scen = h->cfg.scenario;
    if (scen != PW_SIMPLE_SPREAD && scen != PW_SIMPLE_TAG)
        return fail(PW_EINVAL, "pw_policy_rollout serves simple_spread, simple_tag and simple_reference");
    if (io->act_idx || io->act_vec || io->act_comm || io->coll)
        return fail(PW_EINVAL, "pw_policy_rollout produces the actions itself (act_out) and has no coll output");
    const bool have_sink = sink && sink->ring;   // a ring: its planes join the alignment check below
    if (!sink_takes(sink) && (!act_out || !io->obs || !io->rew || !io->rew_shared || !io->done || !io->terminal))
        return fail(PW_EINVAL, "without a sink (a ring or the episode bookkeeping), act_out and the obs, rew, rew_shared, done, terminal outputs are required");
    if (sink) {
        // a full row is not a function of the stored state alone for every configuration served here: the single-head row ring only
        // (shared-reward or per-agent)
        if (int rc = row_ring_only(sink->ring, "pw_policy_rollout sink (generic form)")) return rc;
        if (int rc = sink_fits(sink, kp.N, kp.D, (int64_t)num_steps * kp.B)) return rc;
    }
    if ((reinterpret_cast<uintptr_t>(io->obs) | reinterpret_cast<uintptr_t>(io->final_obs) | reinterpret_cast<uintptr_t>(frag) |
         reinterpret_cast<uintptr_t>(w_hh_fw) | reinterpret_cast<uintptr_t>(w_hh_bw) |
         (have_sink ? reinterpret_cast<uintptr_t>(sink->ring->next_obs) | reinterpret_cast<uintptr_t>(sink->ring->obs) : 0)) & 15)
        return fail(PW_EINVAL, "obs, final_obs, frag, w_hh and the ring planes must be 16-byte aligned");
    if (h->actor_bf16x3) return fail(PW_EINVAL, "PW_ACTOR_BF16X3 serves the simple_spread rollout in its third form (and pw_actor_fused) only");
    const int obs_mode = scen == PW_SIMPLE_SPREAD ? h->cfg.obs_mode : PW_OBS_LOCAL;
    const int E = pw_policy_generic_envs_per_workgroup(scen, obs_mode, kp.N, kp.L, kp.A);
    if (E < 1)
        return fail(PW_EINVAL, "pw_policy_rollout, generic form: N = " + std::to_string(kp.N) + " agents with observation rows of D = " +
                                   std::to_string(kp.D) + " numbers do not fit: rows of at most 64 numbers, at most 96 rows and 160 KB of LDS per workgroup");
    PolicyRolloutGenericArgs P;
    std::memset(&P, 0, sizeof(P));
    P.A = actor_args(frag, b1, b_ih, w_hh_fw, w_hh_bw, w2, b2, kp.B, kp.N, kp.D, relu_out, 5, 0, seed, step, step_dev);
    P.A.E = E;
    P.K = kp;
    P.obs = io->obs; P.final_obs = io->final_obs; P.rew = io->rew; P.rew_shared = io->rew_shared;
    P.done = io->done; P.terminal = io->terminal;
    P.T = num_steps; P.act_out = act_out;
    sink_into(P.sink, sink);
    const int S1C = (kp.D + 7) / 8;
    const size_t shm = policy_generic_lds(4 * S1C, kp.D, E, kp.N, kp.L).bytes;
    const unsigned grid = (unsigned)((kp.B + E - 1) / E);
    hipStream_t st = static_cast<hipStream_t>(stream);
#define PW_PG3(SC, OB, C, SK)                                                                                            \
    do {                                                                                                                 \
        static unsigned long long attr_set = 0; /* bit = device */                                                       \
        PW_LDS_OPTIN(&attr_set, (pw_policy_rollout_generic_kernel<SC, OB, C, SK>));                                      \
        hipLaunchKernelGGL((pw_policy_rollout_generic_kernel<SC, OB, C, SK>), dim3(grid), dim3(512), shm, st, P);        \
    } while (0)
#define PW_PG(SC, OB, C) case C: if (sink) PW_PG3(SC, OB, C, true); else PW_PG3(SC, OB, C, false); break;
#define PW_PG_ALL(SC, OB) switch (S1C) { PW_PG(SC, OB, 1) PW_PG(SC, OB, 2) PW_PG(SC, OB, 3) PW_PG(SC, OB, 4) PW_PG(SC, OB, 5) PW_PG(SC, OB, 6) PW_PG(SC, OB, 7) PW_PG(SC, OB, 8) }
    if (scen == PW_SIMPLE_TAG) PW_PG_ALL(PW_SIMPLE_TAG, PW_OBS_LOCAL)
    else if (obs_mode == PW_OBS_FULL) PW_PG_ALL(PW_SIMPLE_SPREAD, PW_OBS_FULL)
    else PW_PG_ALL(PW_SIMPLE_SPREAD, PW_OBS_LOCAL)
#undef PW_PG_ALL
#undef PW_PG
#undef PW_PG3
    PW_HIP_CHECK(hipGetLastError());
    h->last_kernel = "pw_policy_rollout_generic_kernel";
    return PW_OK;
}

}  // extern "C"
