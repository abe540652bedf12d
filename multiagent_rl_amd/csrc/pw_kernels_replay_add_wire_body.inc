// The body of pw_replay_add_wire_kernel and pw_replay_add_wire_agents_kernel (pw_kernels_replay.hpp), included once in each: PW_WIRE_PA is the ring's kind
// (false: the shared ring, true: a per-agent ring) and PW_WIRE_REW the trailer plane rew [T,B,N] (nullptr for the shared ring); the reward /
// done store (PW_WIRE_REWARD) is the only difference between the two.
    typedef float vec_t __attribute__((ext_vector_type(V)));
    const WirePtrs p = wire_ptrs(w, const_cast<void *>(wire));
    const int ND = w.N * w.D, N = w.N, NDV = ND / V;
    const size_t per_step = (size_t)w.B * NDV, total = (size_t)w.T * per_step;
    const vec_t *obs0 = reinterpret_cast<const vec_t *>(p.obs0), *obs = reinterpret_cast<const vec_t *>(p.obs);
    const vec_t *fin = reinterpret_cast<const vec_t *>(p.final_rows);
    vec_t *r_obs = reinterpret_cast<vec_t *>(st.obs), *r_next = reinterpret_cast<vec_t *>(st.next_obs);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t t = i / per_step, rem = i - t * per_step, e = rem / NDV, c = rem - e * NDV;
        const size_t te = t * w.B + e;
        const size_t slot = (size_t)((start + (int64_t)te) % st.capacity);
        r_obs[slot * NDV + c] = t == 0 ? obs0[rem] : obs[i - per_step];
        const unsigned fs = p.fin_slot[te];
        r_next[slot * NDV + c] = fs != 0xFFu ? fin[(size_t)fs * per_step + rem] : obs[i];
        for (int q = 0; q < V; ++q) {
            const size_t cc = c * V + q;
            if (cc < (size_t)N) {
                st.act[slot * N + cc] = p.act[te * N + cc];
                PW_WIRE_REWARD(N, cc, false);
            }
        }
        if (!PW_WIRE_PA) PW_WIRE_REWARD(N, 0, c == 0);
    }
