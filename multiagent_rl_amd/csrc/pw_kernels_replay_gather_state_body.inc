// pw_kernels_replay_gather_state_body.inc -- the body of pw_replay_gather_state_kernel, included once per kernel of pw_kernels_replay.hpp
// that gathers from a STATE ring.  In scope: as pw_kernels_replay_gather_body.inc.
    const RowGeom G = {st.scenario, st.num_agents, st.num_landmarks, st.num_adversaries};
    const int N = st.num_agents, U = st.obs_dim / 2, W0 = st.head_width[0] > 0 ? st.head_width[0] : 5;
    const size_t total = (size_t)b * N * U;
    const float4 *r_s = reinterpret_cast<const float4 *>(st.obs), *r_n = reinterpret_cast<const float4 *>(st.next_obs);
    const float2 *r_lm = reinterpret_cast<const float2 *>(st.lm);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t ea = i / U, e = ea / N;
        const int k = (int)(i - ea * U), a = (int)(ea - e * N);
        const size_t slot = PW_GATHER_SLOT(e);
        PW_GATHER_NOTE(k == 0 && a == 0, e, slot)
        const float2 *lm = r_lm + slot * G.L;
        if (out_obs) reinterpret_cast<float2 *>(out_obs)[i] = state_row_unit(G, a, k, r_s + slot * N, lm);
        if (out_next_obs) reinterpret_cast<float2 *>(out_next_obs)[i] = state_row_unit(G, a, k, r_n + slot * N, lm);
        if (k == 0) {
            if (out_act) {
                const int a0 = st.act[slot * N + a];
                float *row = out_act + ea * W0;
                for (int q = 0; q < W0; ++q) row[q] = a0 == q ? 1.0f : 0.0f;
            }
            if (st.per_agent) {  // the BiCNet tuple: planes [cap,N] -> [b,N]
                if (out_rew) out_rew[ea] = st.rew[slot * N + a];
                if (out_done) out_done[ea] = st.done[slot * N + a];
            } else if (a == 0) {
                if (out_rew) out_rew[e] = st.rew[slot];
                if (out_done) out_done[e] = st.done[slot];
            }
        }
    }
