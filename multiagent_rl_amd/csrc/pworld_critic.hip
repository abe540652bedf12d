// libpworld.so, third translation unit -- the learner's critic forward and TD target (rls/model/ac_network_multi_gumbel.py
// CriticNetwork, ddpg_gumbel_fix.py:148-154): pw_critic_forward; and the BiCNet baseline's per-step critic with its per-agent TD
// target (ac_network_multi_gumbel_BIC.py CriticNetwork, BIC_gumbel_fix.py:155-160): pw_critic_forward_steps; and the model-learning
// variant's two-head critic (ac_network_model_multi_gumbel.py CriticNetwork, model_ddpg_gumbel_fix.py:158-163): pw_critic_forward_model.  The kernel is csrc/pw_kernels_critic.hpp; the gate functions
// and the LDS barrier are the actor's (pw_lstm_math.hpp: included, not copied).  Declared in include/pworld.h; the error text
// is shared with pworld.hip.
#include "pw_host.hpp"
#include "pw_lstm_math.hpp"
#include "pw_kernels_critic.hpp"

namespace {

// One trait per form: the argument block, the kernel of <KO, KA>, its LDS bytes and the rows per workgroup (R).
template <class Args> using CriticKernel = void (*)(const Args);

struct AttentionForm {  // pw_critic_forward
    using Args = CriticArgs;
    template <int KO, int KA> static CriticKernel<Args> kernel() { return pw_critic_forward_kernel<KO, KA, false>; }
    static size_t lds(const CriticArgs &C) { return critic_lds(C.N, C.R).bytes; }
    static int rows(int N) { return N <= 32 ? 16 : 8; }  // all N step outputs of a workgroup's rows stay in LDS for the attention pass
};

struct StepsForm {  // pw_critic_forward_steps
    using Args = CriticArgs;
    template <int KO, int KA> static CriticKernel<Args> kernel() { return pw_critic_forward_kernel<KO, KA, true>; }
    static size_t lds(const CriticArgs &C) { return critic_steps_lds(C.N, C.R).bytes; }
    static int rows(int) { return 16; }  // only h_{t-1} and h_t are live: the two-slot ring serves every N with full tiles
};

struct ModelForm : AttentionForm {  // pw_critic_forward_model: the attention form's LDS layout and R rule
    using Args = CriticModelArgs;
    template <int KO, int KA> static CriticKernel<Args> kernel() { return pw_critic_forward_kernel<KO, KA>; }
};

// The one launcher.  optin_mask is a static of the instantiation, so there is one per kernel: a mask two kernels shared would
// skip the opt-in of the second, whose launch then fails wherever its LDS exceeds 64 KB.
template <class Form, int KO, int KA>
int critic_launch(const typename Form::Args &C, hipStream_t stream)
{
    static unsigned long long optin_mask = 0;
    const auto kernel = Form::template kernel<KO, KA>();
    PW_LDS_OPTIN(&optin_mask, kernel);
    const long groups = (C.b + C.R - 1) / C.R;
    hipLaunchKernelGGL(kernel, dim3((unsigned)groups), dim3(512), Form::lds(C), stream, C);
    PW_HIP_CHECK(hipGetLastError());
    return PW_OK;
}

template <class Form, int KO>
int critic_ka(const typename Form::Args &C, hipStream_t s)
{
    return (C.A + 3) / 4 <= 2 ? critic_launch<Form, KO, 2>(C, s) : critic_launch<Form, KO, 4>(C, s);
}

// The one ladder: R by the form's rule, then the instantiation by the k steps of dense1 (four k each): observation part
// (so <= 26), action part (<= 4).
template <class Form>
int critic_go(typename Form::Args &C, void *stream)
{
    C.R = Form::rows(C.N);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int so = (C.D + 3) / 4;
    if (so <= 4) return critic_ka<Form, 4>(C, s);
    if (so <= 8) return critic_ka<Form, 8>(C, s);
    if (so <= 16) return critic_ka<Form, 16>(C, s);
    return critic_ka<Form, 26>(C, s);
}

// the arguments all entry points share; fills everything of C but R
int critic_args(const float *obs, const int32_t *act_idx, const float *act_vec, int32_t n_act0, int32_t n_act1, const float *w1,
                const float *b1, const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh, const float *w2,
                const float *b2, int64_t b, int32_t N, int32_t obs_dim, const float *rew, const float *done, float gamma, float *q,
                float *y, CriticArgs &C)
{
    if (!obs || !w1 || !b1 || !w_ih || !w_hh || !b_ih || !b_hh || !w2 || !b2 || !q) return fail(PW_EINVAL, "null argument");
    if ((act_idx != nullptr) == (act_vec != nullptr)) return fail(PW_EINVAL, "exactly one of act_idx / act_vec must be given");
    if (n_act0 < 1 || n_act1 < 0 || n_act0 + n_act1 > 16)
        return fail(PW_EINVAL, "action widths: n_act0 >= 1, n_act0 + n_act1 <= 16");
    if (N < 1 || N > PW_MAX_AGENTS) return fail(PW_EINVAL, "N must be in [1, 64]");
    if (obs_dim < 1 || obs_dim > 104) return fail(PW_EINVAL, "obs_dim must be in [1, 104]");
    if (b < 1 || b > (int64_t)0x7fffffff) return fail(PW_EINVAL, "b must be in [1, 2^31)");
    if (y ? (!rew || !done) : (rew || done)) return fail(PW_EINVAL, "the TD target needs rew, done and y together");
    C.obs = obs; C.act_idx = act_idx; C.act_vec = act_vec;
    C.w1 = w1; C.b1 = b1; C.w_ih = w_ih; C.w_hh = w_hh; C.b_ih = b_ih; C.b_hh = b_hh; C.w2 = w2; C.b2 = b2;
    C.rew = rew; C.done = done; C.q = q; C.y = y;
    C.b = (long)b; C.N = N; C.D = obs_dim; C.A = n_act0 + n_act1; C.n0 = n_act0; C.n1 = n_act1;
    C.gamma = gamma;
    return PW_OK;
}

}  // namespace

extern "C" {

int pw_critic_forward(const float *obs, const int32_t *act_idx, const float *act_vec, int32_t n_act0, int32_t n_act1,
                      const float *w1, const float *b1, const float *w_ih, const float *w_hh, const float *b_ih,
                      const float *b_hh, const float *w2, const float *b2, int64_t b, int32_t N, int32_t obs_dim,
                      const float *rew, const float *done, float gamma, float *q, float *y, void *stream)
{
    CriticArgs C;
    if (int rc = critic_args(obs, act_idx, act_vec, n_act0, n_act1, w1, b1, w_ih, w_hh, b_ih, b_hh, w2, b2, b, N, obs_dim, rew, done,
                             gamma, q, y, C))
        return rc;
    return critic_go<AttentionForm>(C, stream);
}

int pw_critic_forward_steps(const float *obs, const int32_t *act_idx, const float *act_vec, int32_t n_act0, int32_t n_act1,
                            const float *w1, const float *b1, const float *w_ih, const float *w_hh, const float *b_ih,
                            const float *b_hh, const float *w2, const float *b2, int64_t b, int32_t N, int32_t obs_dim,
                            const float *rew, const float *done, float gamma, float *q, float *y, void *stream)
{
    CriticArgs C;
    if (int rc = critic_args(obs, act_idx, act_vec, n_act0, n_act1, w1, b1, w_ih, w_hh, b_ih, b_hh, w2, b2, b, N, obs_dim, rew, done,
                             gamma, q, y, C))
        return rc;
    return critic_go<StepsForm>(C, stream);
}

int pw_critic_forward_model(const float *obs, const int32_t *act_idx, const float *act_vec, int32_t n_act0, int32_t n_act1,
                            const float *w1, const float *b1, const float *w_ih, const float *w_hh, const float *b_ih,
                            const float *b_hh, const float *w2, const float *b2, const float *w3, const float *b3, int64_t b,
                            int32_t N, int32_t obs_dim, const float *rew, const float *done, float gamma, float *q, float *r_pred,
                            float *y, void *stream)
{
    CriticModelArgs C;
    if (int rc = critic_args(obs, act_idx, act_vec, n_act0, n_act1, w1, b1, w_ih, w_hh, b_ih, b_hh, w2, b2, b, N, obs_dim, rew, done,
                             gamma, q, y, C))
        return rc;
    if (r_pred && (!w3 || !b3)) return fail(PW_EINVAL, "the reward prediction needs w3 and b3");
    C.w3 = w3; C.b3 = b3; C.r_pred = r_pred;
    return critic_go<ModelForm>(C, stream);
}

}  // extern "C"
