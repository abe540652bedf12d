// pw_kernels_optim_adam_body.inc -- the body of pw_adam_step_kernel, included by that kernel (pw_kernels_optim.hpp) and by pw_adam_step_dev_kernel
// (pw_kernels_optim_dev.hpp, which says why it is text and not a function).  In scope where it is included: the argument block A (OptArgs), s_part (kOptThreads doubles of LDS)
// and the two step-dependent scalars as the macros PW_ADAM_BC2_SQRT / PW_ADAM_STEP_SIZE.
    const int lane = threadIdx.x;
    float coef = 1.0f;
    if (A.need_norm) {
        double acc = 0.0;
        for (int k = 0; k < A.count; ++k) {
            const float *__restrict__ g = A.t[k].grad;
            const long n = A.t[k].numel;
            for (long i = lane; i < n; i += kOptThreads) {
                const double x = (double)g[i];
                acc += x * x;
            }
        }
        s_part[lane] = acc;
        __syncthreads();
        for (int s = kOptThreads / 2; s > 0; s >>= 1) {
            if (lane < s) s_part[lane] += s_part[lane + s];
            __syncthreads();
        }
        const double norm = sqrt(s_part[0]);
        if (A.max_norm > 0.0) {
            const double c = A.max_norm / (norm + 1e-6);
            coef = (float)(c >= 1.0 ? 1.0 : c);   // NaN passes, as torch's clamp(max=1) lets it
        }
        if (A.total_norm != nullptr && blockIdx.x == 0 && lane == 0) *A.total_norm = (float)norm;
    }
    const int k = opt_tile_owner(A, (int)blockIdx.x);
    const OptTensor T = A.t[k];
    const long base = (long)((int)blockIdx.x - A.tile_begin[k]) * kOptTile;
    const bool clip = A.max_norm > 0.0;
#pragma unroll
    for (int j = 0; j < kOptTile / kOptThreads; ++j) {
        const long i = base + j * kOptThreads + lane;
        if (i >= T.numel) break;
        float g = T.grad[i];
        float p = T.param[i];
        if (clip) g = g * coef;
        if (A.wd != 0.0f) g = __builtin_fmaf(A.wd, p, g);
        const float m = __builtin_fmaf(T.exp_avg[i], A.beta1, g * A.omb1);
        const float v = __builtin_fmaf(T.exp_avg_sq[i], A.beta2, (g * g) * A.omb2);
        const float d = sqrtf(v) / PW_ADAM_BC2_SQRT + A.eps;
        p = __builtin_fmaf(-PW_ADAM_STEP_SIZE, m / d, p);
        T.exp_avg[i] = m;
        T.exp_avg_sq[i] = v;
        T.param[i] = p;
        if (T.target != nullptr) T.target[i] = A.hard ? p : opt_polyak(T.target[i], p, A.omt, A.tau);
    }
