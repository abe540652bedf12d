// The body of pw_replay_add_state_wire_to_state_ring_kernel and pw_replay_add_state_wire_to_state_ring_agents_kernel (pw_kernels_replay.hpp), included once in each: PW_WIRE_PA is the ring's kind
// (false: the shared ring, true: a per-agent ring) and PW_WIRE_REW the trailer plane rew [T,B,N] (nullptr for the shared ring); the reward /
// done store (PW_WIRE_REWARD) is the only difference between the two.
    const StateWirePtrs p = state_wire_ptrs(w, const_cast<void *>(wire));
    const int N = w.N, L = w.L;
    const size_t BN = (size_t)w.B * N, total = (size_t)w.T * BN;
    float4 *r_s = reinterpret_cast<float4 *>(st.obs), *r_n = reinterpret_cast<float4 *>(st.next_obs);
    float2 *r_lm = reinterpret_cast<float2 *>(st.lm);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t t = i / BN, ea = i - t * BN, e = ea / N;
        const int a = (int)(ea - e * N);
        const size_t te = t * w.B + e;
        const unsigned epi = p.epi[te], ke = epi & 0x7fu;
        const size_t slot = (size_t)((start + (int64_t)te) % st.capacity);
        r_s[slot * N + a] = t == 0 ? p.state0[ea] : p.state[(t - 1) * BN + ea];
        r_n[slot * N + a] = (epi & 0x80u) ? p.final_state[(size_t)ke * BN + ea] : p.state[t * BN + ea];
        const float2 *lm = p.lm + ((size_t)ke * w.B + e) * L;
        for (int l = a; l < L; l += N) r_lm[slot * L + l] = lm[l];
        st.act[slot * N + a] = p.act[te * N + a];
        PW_WIRE_REWARD(N, a, a == 0);
    }
