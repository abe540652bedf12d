// The body of pw_replay_add_ref_wire_kernel and pw_replay_add_ref_wire_agents_kernel (pw_kernels_replay.hpp), included once in each: PW_WIRE_PA is the ring's kind
// (false: the shared ring, true: a per-agent ring) and PW_WIRE_REW the trailer plane rew [T,B,N] (nullptr for the shared ring); the reward /
// done store (PW_WIRE_REWARD) is the only difference between the two.
    const RefWirePtrs p = ref_wire_ptrs(w, const_cast<void *>(wire));
    const size_t BN = (size_t)w.B * kRefN, per_step = BN * kRefD, total = (size_t)w.T * per_step;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t t = i / per_step, rem = i - t * per_step, ea = rem / kRefD, e = ea / kRefN;
        const int c = (int)(rem - ea * kRefD), a = (int)(ea - e * kRefN);
        const size_t te = t * w.B + e, other = e * kRefN + (1 - a);
        const unsigned epi = p.epi[te], k = epi & 0x7fu;
        const bool ended = (epi & 0x80u) != 0;
        float o, n;
        if (c < kRefHead) {
            o = (t == 0 ? p.head0 : p.head + (t - 1) * BN * kRefHead)[ea * kRefHead + c];
            n = (ended ? p.final_head + (size_t)k * BN * kRefHead : p.head + t * BN * kRefHead)[ea * kRefHead + c];
        } else if (c < kRefHead + 3) {
            o = n = (c - kRefHead) == (int)p.goal[(size_t)k * BN + ea] ? 0.75f : 0.25f;   // one episode: obs_t and next_obs_t share the goal
        } else {
            const int q = c - kRefHead - 3;
            // what agent a sees of the other agent at step t: the symbol it sampled at step t - 1 (none right after a reset)
            const unsigned prev = t == 0 ? p.comm0[ea] : ((p.epi[te - w.B] & 0x80u) ? 0xFFu : p.act[((t - 1) * BN + other) * 2 + 1]);
            o = (unsigned)q == prev ? 1.0f : 0.0f;
            n = q == (int)p.act[(t * BN + other) * 2 + 1] ? 1.0f : 0.0f;   // pre-reset or not: this step's symbol
        }
        const size_t slot = (size_t)((start + (int64_t)te) % st.capacity);
        const size_t at = (slot * kRefN + a) * kRefD + c;
        st.obs[at] = o;
        st.next_obs[at] = n;
        if (c < 2) st.act[(slot * kRefN + a) * 2 + c] = p.act[(t * BN + ea) * 2 + c];
        if (c == 0) PW_WIRE_REWARD(kRefN, a, a == 0);
    }
