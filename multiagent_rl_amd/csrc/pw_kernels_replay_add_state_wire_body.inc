// The body of pw_replay_add_state_wire_kernel and pw_replay_add_state_wire_agents_kernel (pw_kernels_replay.hpp), included once in each: PW_WIRE_PA is the ring's kind
// (false: the shared ring, true: a per-agent ring) and PW_WIRE_REW the trailer plane rew [T,B,N] (nullptr for the shared ring); the reward /
// done store (PW_WIRE_REWARD) is the only difference between the two.
    typedef float vec_t __attribute__((ext_vector_type(V)));
    const StateWirePtrs p = state_wire_ptrs(w, const_cast<void *>(wire));
    const int N = w.N, L = w.L, CH = w.D / V;
    const size_t BN = (size_t)w.B * N, per_step = BN * CH, total = (size_t)w.T * per_step;
    vec_t *r_obs = reinterpret_cast<vec_t *>(st.obs), *r_next = reinterpret_cast<vec_t *>(st.next_obs);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t t = i / per_step, rem = i - t * per_step, ea = rem / CH, e = ea / N;
        const int c = (int)(rem - ea * CH), a = (int)(ea - e * N);
        const size_t te = t * w.B + e;
        const unsigned epi = p.epi[te], k = epi & 0x7fu;
        const float4 s_obs = t == 0 ? p.state0[ea] : p.state[(t - 1) * BN + ea];
        const float4 s_next = (epi & 0x80u) ? p.final_state[(size_t)k * BN + ea] : p.state[t * BN + ea];
        const float2 *lm = p.lm + ((size_t)k * w.B + e) * L;
        vec_t o, n;
        if (V == 4) {
            if (c == 0) {
                o[0] = s_obs.x; o[1] = s_obs.y; o[2] = s_obs.z; o[3] = s_obs.w;
                n[0] = s_next.x; n[1] = s_next.y; n[2] = s_next.z; n[3] = s_next.w;
            } else {
                const float2 l0 = lm[2 * c - 2], l1 = lm[2 * c - 1];
                o[0] = l0.x - s_obs.z; o[1] = l0.y - s_obs.w; o[2] = l1.x - s_obs.z; o[3] = l1.y - s_obs.w;
                n[0] = l0.x - s_next.z; n[1] = l0.y - s_next.w; n[2] = l1.x - s_next.z; n[3] = l1.y - s_next.w;
            }
        } else {
            if (c == 0) { o[0] = s_obs.x; o[1] = s_obs.y; n[0] = s_next.x; n[1] = s_next.y; }
            else if (c == 1) { o[0] = s_obs.z; o[1] = s_obs.w; n[0] = s_next.z; n[1] = s_next.w; }
            else {
                const float2 l0 = lm[c - 2];
                o[0] = l0.x - s_obs.z; o[1] = l0.y - s_obs.w;
                n[0] = l0.x - s_next.z; n[1] = l0.y - s_next.w;
            }
        }
        const size_t slot = (size_t)((start + (int64_t)te) % st.capacity);
        const size_t at = (slot * N + a) * CH + c;
        r_obs[at] = o;
        r_next[at] = n;
        if (c == 0) {
            st.act[slot * N + a] = p.act[te * N + a];
            PW_WIRE_REWARD(N, a, a == 0);
        }
    }
