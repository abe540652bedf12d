// pw_kernels_critic_body.inc -- the body of pw_critic_forward_kernel, included once per kernel template of pw_kernels_critic.hpp
// (which says why it is text and not a function).  In scope where it is included: KO, KA, STEPS, MODEL (compile-time) and the
// kernel's argument block C (CriticArgs; CriticModelArgs where MODEL).
    constexpr int KS = KO + KA;
    extern __shared__ __attribute__((aligned(16))) unsigned char critic_smem[];
    const int tid = threadIdx.x, lane = tid & 63, n16 = lane & 15, kq = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int hq = wave & 3, grp = wave >> 2;
    const int N = C.N, D = C.D, A = C.A, K = D + A, R = C.R, FR = 4 * R;
    const auto Y = critic_layout<STEPS>(N, R, critic_smem);
    const long b0 = (long)blockIdx.x * R;
    const int rows_here = (int)(C.b - b0 < (long)R ? C.b - b0 : (long)R);
    const bool col_ok = n16 < rows_here;  // columns past the rows of this workgroup compute on row b0 and store nothing
    const int nq = col_ok ? n16 : 0;
    const int slot = kq * R + nq;
    const int heads = C.n1 > 0 ? 2 : 1;

    // ---- stationary weights: the wave's two LSTM tiles and its dense1 tile
    float aih[2][16], ahh[2][16], bias[2][4], a1[KS], b1v[4];
#pragma unroll
    for (int T = 0; T < 2; ++T) {
        const int wrow = (n16 & 3) * 64 + wave * 8 + 4 * T + (n16 >> 2);  // gate * 64 + unit
#pragma unroll
        for (int sx = 0; sx < 16; ++sx) {
            aih[T][sx] = C.w_ih[wrow * 64 + 4 * sx + kq];
            ahh[T][sx] = C.w_hh[wrow * 64 + 4 * sx + kq];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {  // accumulator role: row group = kq = unit within the tile, register = gate
            const int r = i * 64 + wave * 8 + 4 * T + kq;
            bias[T][i] = C.b_ih[r] + C.b_hh[r];
        }
    }
    const float *w1o = C.w1 + (16 * hq + n16) * K + kq, *w1a = w1o + D;
    auto w1_frag = [&](const int sx) {  // k step sx < KO: observation column 4 sx + kq; else action column 4 (sx - KO) + kq
        if (sx < KO) return 4 * sx + kq < D ? w1o[4 * sx] : 0.0f;
        return 4 * (sx - KO) + kq < A ? w1a[4 * (sx - KO)] : 0.0f;
    };
#pragma unroll
    for (int sx = 0; sx < KS; ++sx) a1[sx] = w1_frag(sx);
#pragma unroll
    for (int i = 0; i < 4; ++i) b1v[i] = C.b1[16 * hq + 4 * kq + i];
    // per-step head: w2 in the order of a lane's B fragments (element e of fragment j = unit 16 j + 4 e + kq)
    float w2v[16], b2v = 0.0f;   // dead (and removed) in the attention instantiations
    if constexpr (STEPS) {
#pragma unroll
        for (int u = 0; u < 16; ++u) w2v[u] = C.w2[16 * (u >> 2) + 4 * (u & 3) + kq];
        b2v = C.b2[0];
    }
    auto out_slot = [](const int t) { return STEPS ? (t & 1) : t; };
    // q_tq of the workgroup's rows from the fragments of h_tq (one wave): 16 units per lane in ascending order, the four k quarters meet
    auto head = [&](const int tq, const float4 (&hv)[4]) {
        float p = 0.0f;
#pragma unroll
        for (int jx = 0; jx < 4; ++jx) {
            p += hv[jx].x * w2v[4 * jx + 0];
            p += hv[jx].y * w2v[4 * jx + 1];
            p += hv[jx].z * w2v[4 * jx + 2];
            p += hv[jx].w * w2v[4 * jx + 3];
        }
        p += lane_xor16(p);
        p += lane_xor32(p);
        if constexpr (STEPS) {
            if (kq == 0 && n16 < R) Y.s_q[n16 * N + tq] = p + b2v;
        }
    };

    // B operands of one dense1 tile: [obs | action] of row (b0 + nq, ts)
    auto load_x = [&](const int ts, float (&xb)[KS]) {
        const size_t row = (size_t)(b0 + nq) * N + ts;
        const float *xo = C.obs + row * D + kq;
#pragma unroll
        for (int sx = 0; sx < KO; ++sx) xb[sx] = 4 * sx + kq < D ? xo[4 * sx] : 0.0f;
        if (C.act_idx) {
            int i0 = C.act_idx[row * heads], i1 = -1;
            i0 = (i0 >= 0 && i0 < C.n0) ? i0 : -1;
            if (heads == 2) {
                i1 = C.act_idx[row * heads + 1];
                i1 = (i1 >= 0 && i1 < C.n1) ? C.n0 + i1 : -1;
            }
#pragma unroll
            for (int sx = 0; sx < KA; ++sx) xb[KO + sx] = (4 * sx + kq == i0 || 4 * sx + kq == i1) ? 1.0f : 0.0f;
        } else {
            const float *xa = C.act_vec + row * A + kq;
#pragma unroll
            for (int sx = 0; sx < KA; ++sx) xb[KO + sx] = 4 * sx + kq < A ? xa[4 * sx] : 0.0f;
        }
    };
    // relu(W1 x + b1) of the wave's hidden quarter -> x1 buffer ts % 4.  Register i of row group kq is hidden unit
    // 16 hq + 4 kq + i: fragment j = hq, element kq, slot (i, n)
    auto dense1 = [&](const int ts, const float (&xb)[KS]) {
        f32x4 acc1 = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int sx = 0; sx < KS; ++sx) acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[sx], xb[sx], acc1, 0, 0, 0);
        if (n16 < R) {
            float *dst = reinterpret_cast<float *>(Y.s_x + ((ts & 3) * 4 + hq) * FR) + kq;
#pragma unroll
            for (int i = 0; i < 4; ++i) dst[(i * R + n16) * 4] = relu_fwd(acc1[i] + b1v[i]);
        }
    };
    // bias + W_ih x1(ts) for the wave's two tiles
    auto inproj = [&](const int ts, f32x4 (&acc)[2]) {
        const float4 *xf = Y.s_x + ((ts & 3) * 4) * FR + slot;
        const float4 xq[4] = {xf[0], xf[FR], xf[2 * FR], xf[3 * FR]};
#pragma unroll
        for (int T = 0; T < 2; ++T) acc[T] = f32x4{bias[T][0], bias[T][1], bias[T][2], bias[T][3]};
#pragma unroll
        for (int jx = 0; jx < 4; ++jx) {
            const float4 bq = xq[jx];
            acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(aih[0][4 * jx + 0], bq.x, acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(aih[1][4 * jx + 0], bq.x, acc[1], 0, 0, 0);
            acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(aih[0][4 * jx + 1], bq.y, acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(aih[1][4 * jx + 1], bq.y, acc[1], 0, 0, 0);
            acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(aih[0][4 * jx + 2], bq.z, acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(aih[1][4 * jx + 2], bq.z, acc[1], 0, 0, 0);
            acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(aih[0][4 * jx + 3], bq.w, acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(aih[1][4 * jx + 3], bq.w, acc[1], 0, 0, 0);
        }
    };

    // ---- prologue: x1 of timesteps 0 and 1
    {
        float xb[KS];
        if (grp < N) {
            load_x(grp, xb);
            dense1(grp, xb);
        }
    }
    wg_lds_barrier();

    // ---- the LSTM, one timestep per barrier
    f32x4 acc[2], accn[2];
    float c0 = 0.f, c1 = 0.f;
    inproj(0, acc);
    for (int t = 0; t < N; ++t) {
        const int ts2 = t + 2 + grp;
        const bool d1_now = !(t & 1) && ts2 < N;  // wave-uniform
        float xb[KS];
        if (d1_now) load_x(ts2, xb);
        if (t > 0) {
            const float4 *hx = Y.s_out + (out_slot(t - 1) * 4) * FR + slot;
            const float4 hv[4] = {hx[0], hx[FR], hx[2 * FR], hx[3 * FR]};
#pragma unroll
            for (int jx = 0; jx < 4; ++jx) {
                const float4 bq = hv[jx];
                acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(ahh[0][4 * jx + 0], bq.x, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(ahh[1][4 * jx + 0], bq.x, acc[1], 0, 0, 0);
                acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(ahh[0][4 * jx + 1], bq.y, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(ahh[1][4 * jx + 1], bq.y, acc[1], 0, 0, 0);
                acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(ahh[0][4 * jx + 2], bq.z, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(ahh[1][4 * jx + 2], bq.z, acc[1], 0, 0, 0);
                acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(ahh[0][4 * jx + 3], bq.w, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(ahh[1][4 * jx + 3], bq.w, acc[1], 0, 0, 0);
            }
            if constexpr (STEPS) {
                if (wave == ((t - 1) & 7)) head(t - 1, hv);   // behind the matrix instructions, before this step's barrier (see INVARIANT)
            }
        }
        // the two cells of this lane: accumulator registers = gates i, f, g, o of unit 8 wave + 4 T + kq
        float h0v, h1v;
        lstm_cell(acc[0][0], acc[0][1], acc[0][2], acc[0][3], c0, h0v);
        lstm_cell(acc[1][0], acc[1][1], acc[1][2], acc[1][3], c1, h1v);
        // unit 8 wave + 4 T + kq is k quarter kq of k step 2 wave + T: fragment wave / 2, elements 2 (wave % 2) + T of this lane's slot
        if (n16 < R)
            reinterpret_cast<float2 *>(Y.s_out + (out_slot(t) * 4 + (wave >> 1)) * FR + kq * R + n16)[wave & 1] = make_float2(h0v, h1v);
        if (d1_now) dense1(ts2, xb);
        if (t + 1 < N) inproj(t + 1, accn);  // before the barrier: work for the matrix pipe while the workgroup meets
        wg_lds_barrier();                    // h_t of every unit is in LDS
        if (t + 1 < N) { acc[0] = accn[0]; acc[1] = accn[1]; }
    }

    if constexpr (STEPS) {
        // ---- the last step's head, then q (and y) of the workgroup's rows leave as one contiguous run of rows_here * N floats
        if (wave == ((N - 1) & 7)) {
            const float4 *hx = Y.s_out + (out_slot(N - 1) * 4) * FR + slot;
            const float4 hv[4] = {hx[0], hx[FR], hx[2 * FR], hx[3 * FR]};
            head(N - 1, hv);
        }
        wg_lds_barrier();
        const int cnt = rows_here * N;
        const size_t base = (size_t)b0 * N;
        for (int i = tid; i < cnt; i += 512) {
            const float qv = Y.s_q[i];
            C.q[base + i] = qv;
            if (C.y) {  // r + GAMMA * q_next * (1. - d) per agent (BIC_gumbel_fix.py:155-160), left to right, no contraction
                const float gq = C.gamma * qv;
                const float nd = 1.0f - C.done[base + i];
                const float prod = gq * nd;
                C.y[base + i] = C.rew[base + i] + prod;
            }
        }
    } else {
    // ---- attention scores <h_t, h_N>: one timestep per wave and round, a lane sums its 16 units, the four k quarters meet
    {
        const float4 *hn = Y.s_out + ((N - 1) * 4) * FR + slot;
        const float4 hN[4] = {hn[0], hn[FR], hn[2 * FR], hn[3 * FR]};
        for (int t = wave; t < N; t += 8) {
            const float4 *o = Y.s_out + (t * 4) * FR + slot;
            float p = 0.0f;
#pragma unroll
            for (int jx = 0; jx < 4; ++jx) {
                const float4 v = o[jx * FR];
                p += v.x * hN[jx].x;
                p += v.y * hN[jx].y;
                p += v.z * hN[jx].z;
                p += v.w * hN[jx].w;
            }
            p += lane_xor16(p);
            p += lane_xor32(p);
            if (kq == 0) Y.s_sc[t * 16 + n16] = p;
        }
    }
    wg_lds_barrier();

    // ---- softmax over the agents (maximum subtracted), every wave for itself: a lane scans t = kq, kq + 4, ..
    float mx = -INFINITY;
    for (int t = kq; t < N; t += 4) mx = fmaxf(mx, Y.s_sc[t * 16 + n16]);
    mx = fmaxf(mx, lane_xor16(mx));
    mx = fmaxf(mx, lane_xor32(mx));
    float den = 0.0f;
    for (int t = kq; t < N; t += 4) den += expf(Y.s_sc[t * 16 + n16] - mx);
    den += lane_xor16(den);
    den += lane_xor32(den);
    // ---- context of this lane's two units, ReLU (the model-learning critic: none), dense2 (and its dense3)
    float ctx0 = 0.0f, ctx1 = 0.0f;
    for (int t = 0; t < N; ++t) {
        const float w = expf(Y.s_sc[t * 16 + n16] - mx) / den;
        const float2 o = reinterpret_cast<const float2 *>(Y.s_out + (t * 4 + (wave >> 1)) * FR + slot)[wave & 1];
        ctx0 += w * o.x;
        ctx1 += w * o.y;
    }
    auto clamp = [](const float v) { return MODEL ? v : relu_fwd(v); };
    float part = C.w2[8 * wave + kq] * clamp(ctx0) + C.w2[8 * wave + 4 + kq] * clamp(ctx1);
    part += lane_xor16(part);
    part += lane_xor32(part);
    if (kq == 0) Y.s_red[wave * 16 + n16] = part;
    // The reward head's [8 waves][16] partial sums, in the order of q's.  They lie in the first x1 buffer: the ring's last reader
    // (inproj of step N - 1) and last writer (dense1) are behind the loop's final barrier, so critic_lds keeps its size and the
    // one barrier below serves both heads.
    [[maybe_unused]] float *const s_red3 = reinterpret_cast<float *>(Y.s_x);
    [[maybe_unused]] const CriticModelArgs *const CM = critic_model_args(C);   // NULL, and unused, in the other forms
    if constexpr (MODEL) {
        if (CM->r_pred) {
            float part3 = CM->w3[8 * wave + kq] * ctx0 + CM->w3[8 * wave + 4 + kq] * ctx1;
            part3 += lane_xor16(part3);
            part3 += lane_xor32(part3);
            if (kq == 0) s_red3[wave * 16 + n16] = part3;
        }
    }
    wg_lds_barrier();
    if (tid < 16 && col_ok) {
        if constexpr (MODEL) {
            if (CM->r_pred) {
                float rv = s_red3[tid];
#pragma unroll
                for (int w = 1; w < 8; ++w) rv += s_red3[w * 16 + tid];
                rv += CM->b3[0];
                CM->r_pred[b0 + tid] = rv;
            }
        }
        float qv = Y.s_red[tid];
#pragma unroll
        for (int w = 1; w < 8; ++w) qv += Y.s_red[w * 16 + tid];
        qv += C.b2[0];
        C.q[b0 + tid] = qv;
        if (C.y) {  // r + GAMMA * q_next * (1. - d), left to right, no contraction (the unit is compiled with -ffp-contract=off)
            const float gq = C.gamma * qv;
            const float nd = 1.0f - C.done[b0 + tid];
            const float prod = gq * nd;
            C.y[b0 + tid] = C.rew[b0 + tid] + prod;
        }
    }
    }
