// The body of pw_replay_add_state_wire_units_kernel and pw_replay_add_state_wire_units_agents_kernel (pw_kernels_replay.hpp), included once in each: PW_WIRE_PA is the ring's kind
// (false: the shared ring, true: a per-agent ring) and PW_WIRE_REW the trailer plane rew [T,B,N] (nullptr for the shared ring); the reward /
// done store (PW_WIRE_REWARD) is the only difference between the two.
    const StateWirePtrs p = state_wire_ptrs(w, const_cast<void *>(wire));
    const RowGeom G = {w.scenario, w.N, w.L, w.num_adversaries};
    const int N = w.N, U = w.D / 2;
    const size_t BN = (size_t)w.B * N, per_step = BN * U, total = (size_t)w.T * per_step;
    float2 *r_obs = reinterpret_cast<float2 *>(st.obs), *r_next = reinterpret_cast<float2 *>(st.next_obs);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t t = i / per_step, rem = i - t * per_step, ea = rem / U, e = ea / N;
        const int k = (int)(rem - ea * U), a = (int)(ea - e * N);
        const size_t te = t * w.B + e;
        const unsigned epi = p.epi[te], ke = epi & 0x7fu;
        const float4 *s_obs = (t == 0 ? p.state0 : p.state + (t - 1) * BN) + e * N;
        const float4 *s_next = ((epi & 0x80u) ? p.final_state + (size_t)ke * BN : p.state + t * BN) + e * N;
        const float2 *lm = p.lm + ((size_t)ke * w.B + e) * w.L;
        const size_t slot = (size_t)((start + (int64_t)te) % st.capacity);
        const size_t at = (slot * N + a) * U + k;
        r_obs[at] = state_row_unit(G, a, k, s_obs, lm);
        r_next[at] = state_row_unit(G, a, k, s_next, lm);
        if (k == 0) {
            st.act[slot * N + a] = p.act[te * N + a];
            PW_WIRE_REWARD(N, a, a == 0);
        }
    }
