"""Float64 NumPy restatement of the critic (test infrastructure; the product never imports it).

Written from the architecture (``multiagent_rl_amd.critic.CriticNetwork`` / rls/model/ac_network_multi_gumbel.py CriticNetwork):
x1 = relu(W1 [obs | action] + b1); a one-layer LSTM (hidden 64, PyTorch gate order i, f, g, o, zero initial state) over the
agent axis; score_t = <out_t, h_N>; softmax over t; ctx = sum_t w_t out_t; q = W2 relu(ctx) + b2.
"""
import numpy as np

KEYS = ('dense1.module.weight', 'dense1.module.bias', 'lstm.weight_ih_l0', 'lstm.weight_hh_l0', 'lstm.bias_ih_l0',
        'lstm.bias_hh_l0', 'dense2.weight', 'dense2.bias')


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def params_f64(module_or_state_dict):
    sd = module_or_state_dict if isinstance(module_or_state_dict, dict) else module_or_state_dict.state_dict()
    out = {}
    for k in KEYS:
        v = sd[k]
        out[k] = (v.detach().cpu().numpy() if hasattr(v, 'detach') else np.asarray(v)).astype(np.float64)
    return out


def one_hot(idx, heads):
    """int [b,N] (one head) or [b,N,2] -> float32 [b,N,sum(heads)]: the heads' one-hots concatenated."""
    idx = np.asarray(idx)
    if idx.ndim == 2:
        idx = idx[..., None]
    return np.concatenate([np.eye(int(n), dtype=np.float32)[idx[..., h]] for h, n in enumerate(heads)], -1)


def forward_f64(params, obs, act, want_steps=False):
    """params: module / state_dict / params_f64 result; obs [b,N,D], act [b,N,A] (any float dtype) -> q float64 [b]."""
    p = params if (isinstance(params, dict) and params[KEYS[0]].dtype == np.float64 and isinstance(params[KEYS[0]], np.ndarray)) \
        else params_f64(params)
    x = np.concatenate([np.asarray(obs, dtype=np.float64), np.asarray(act, dtype=np.float64)], -1)
    b, N, _ = x.shape
    x1 = np.maximum(x @ p['dense1.module.weight'].T + p['dense1.module.bias'], 0.0)
    wih, whh = p['lstm.weight_ih_l0'], p['lstm.weight_hh_l0']
    bias = p['lstm.bias_ih_l0'] + p['lstm.bias_hh_l0']
    h, c = np.zeros((b, 64)), np.zeros((b, 64))
    steps = np.empty((b, N, 64))
    for t in range(N):
        g = x1[:, t] @ wih.T + h @ whh.T + bias
        i, f, gg, o = _sigmoid(g[:, :64]), _sigmoid(g[:, 64:128]), np.tanh(g[:, 128:192]), _sigmoid(g[:, 192:])
        c = f * c + i * gg
        h = o * np.tanh(c)
        steps[:, t] = h
    score = np.einsum('bnk,bk->bn', steps, h)
    w = np.exp(score - score.max(1, keepdims=True))
    w /= w.sum(1, keepdims=True)
    ctx = np.maximum(np.einsum('bn,bnk->bk', w, steps), 0.0)
    q = ctx @ p['dense2.weight'][0] + p['dense2.bias'][0]
    return (q, steps, score) if want_steps else q


# the fixture's cases and the rule its inputs are drawn by (tests/golden/make_critic_golden.py and the tests share it): the
# legacy NumPy generator is stable across NumPy versions, so critic_forward.npz carries the weights and the outputs only
GOLDEN_CASES = [(6, 16, (5,)), (3, 10, (5,)), (2, 21, (5, 10)), (48, 100, (5,))]
GOLDEN_ROWS = 64


def golden_name(N, D, heads):
    return 'N%d_D%d_h%s' % (N, D, 'x'.join(str(h) for h in heads))


def golden_inputs(N, D, heads, rows=GOLDEN_ROWS):
    """-> obs float32 [rows,N,D] ~ N(0, 1), act_idx int32 [rows,N,len(heads)] uniform."""
    rng = np.random.RandomState(1000 * N + D)
    obs = rng.standard_normal((rows, N, D)).astype(np.float32)
    idx = np.stack([rng.randint(0, n, (rows, N)) for n in heads], -1).astype(np.int32)
    return obs, idx
