// pw_kernels_replay_gather_body.inc -- the body of pw_replay_gather_kernel, included once per kernel of pw_kernels_replay.hpp that
// gathers from a row ring (which says why it is text and not a function).  In scope where it is included: st, b and the five output
// pointers; PW_GATHER_SLOT(e) = the ring slot of batch element e; PW_GATHER_NOTE(first, e, slot) = a statement run with first == true
// by one thread per element (empty for pw_replay_gather).
    const int ND = st.num_agents * st.obs_dim, N = st.num_agents, H = store_heads(st);
    const int W0 = st.head_width[0] > 0 ? st.head_width[0] : 5, W1 = H == 2 ? st.head_width[1] : 0, W = W0 + W1;
    const size_t total = (size_t)b * ND;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t e = i / ND, c = i - e * ND;
        const size_t slot = PW_GATHER_SLOT(e);
        PW_GATHER_NOTE(c == 0, e, slot)
        if (out_obs) out_obs[i] = st.obs[slot * ND + c];
        if (out_next_obs) out_next_obs[i] = st.next_obs[slot * ND + c];
        if (c < (size_t)N) {
            if (out_act) {  // the one-hot rows the reference stored: [head 0 | head 1] per agent (run.py:38-41)
                const int a0 = st.act[(slot * N + c) * H], a1 = H == 2 ? st.act[(slot * N + c) * H + 1] : -1;
                float *row = out_act + (e * N + c) * W;
                for (int k = 0; k < W0; ++k) row[k] = a0 == k ? 1.0f : 0.0f;
                for (int k = 0; k < W1; ++k) row[W0 + k] = a1 == k ? 1.0f : 0.0f;
            }
            if (st.per_agent) {
                if (out_rew) out_rew[e * N + c] = st.rew[slot * N + c];
                if (out_done) out_done[e * N + c] = st.done[slot * N + c];
            }
        }
        if (c == 0 && !st.per_agent) {
            if (out_rew) out_rew[e] = st.rew[slot];
            if (out_done) out_done[e] = st.done[slot];
        }
    }
