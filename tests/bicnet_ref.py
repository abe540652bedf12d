"""Float64 NumPy restatement of the per-step (BiCNet) critic (test infrastructure; the product never imports it).

``multiagent_rl_amd.critic.BiCNetCritic`` / rls/model/ac_network_multi_gumbel_BIC.py CriticNetwork: the front end and the LSTM of
tests/critic_ref.py (its ``forward_f64(want_steps=True)`` gives the step outputs), then q[b, t] = <w2, h_t[b]> + b2 on the LSTM output
itself -- no ReLU, no attention.  The only difference in the parameters is the name of the last layer: ``dense2.module.*``.
"""
import numpy as np

from tests import critic_ref as cr

KEYS = cr.KEYS[:6] + ('dense2.module.weight', 'dense2.module.bias')
_TO_ATTENTION = {'dense2.module.weight': 'dense2.weight', 'dense2.module.bias': 'dense2.bias'}


def params_f64(module_or_state_dict):
    """-> the float64 parameters under tests/critic_ref.py's key names (dense2.module.* -> dense2.*)."""
    sd = module_or_state_dict if isinstance(module_or_state_dict, dict) else module_or_state_dict.state_dict()
    out = {}
    for k in KEYS:
        v = sd[k]
        out[_TO_ATTENTION.get(k, k)] = (v.detach().cpu().numpy() if hasattr(v, 'detach') else np.asarray(v)).astype(np.float64)
    return out


def forward_f64(params, obs, act):
    """params: module / state_dict with the BiCNet keys; obs [b,N,D], act [b,N,A] -> q float64 [b,N]."""
    p = params_f64(params)
    _, steps, _ = cr.forward_f64(p, obs, act, want_steps=True)
    return steps @ p['dense2.weight'][0] + p['dense2.bias'][0]
