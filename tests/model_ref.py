"""Float64 NumPy restatement of the model-learning variant's networks (test infrastructure; the product never imports it).

Written from the architecture (rls/model/ac_network_model_multi_gumbel.py): the critic is the attention critic of tests/critic_ref.py
up to the context -- its LSTM steps are reused, ``critic_ref.forward_f64(..., want_steps=True)`` -- then NO ReLU and two heads,
q = W2 ctx + b2 and r = W3 ctx + b3; the actor is oracle/actor_oracle.py's float64 BiLSTM with a third head on the same ReLU'd
output, next_state = W3 H + b3.
"""
import numpy as np

from oracle import actor_oracle as ao  # checker only
from tests import critic_ref as cr

# the fixture's cases (tests/golden/make_model_golden.py and the tests share them); inputs by critic_ref.golden_inputs
GOLDEN_CASES = [(6, 16, (5,)), (3, 10, (5,)), (2, 21, (5, 10)), (24, 52, (5,))]
ACTOR_CASES = GOLDEN_CASES[:2]   # the two smallest
GOLDEN_FILE = 'model_forward.npz'


def _f64(v):
    return (v.detach().cpu().numpy() if hasattr(v, 'detach') else np.asarray(v)).astype(np.float64)


def critic_f64(module_or_state_dict, obs, act, want_ctx=False):
    """obs [b,N,D], act [b,N,A] -> (q, r) float64 [b] each (``want_ctx``: also the context [b,64], which no ReLU follows)."""
    sd = module_or_state_dict if isinstance(module_or_state_dict, dict) else module_or_state_dict.state_dict()
    _, steps, score = cr.forward_f64(sd, obs, act, want_steps=True)
    w = np.exp(score - score.max(1, keepdims=True))
    w /= w.sum(1, keepdims=True)
    ctx = np.einsum('bn,bnk->bk', w, steps)
    q = ctx @ _f64(sd['dense2.weight'])[0] + _f64(sd['dense2.bias'])[0]
    r = ctx @ _f64(sd['dense3.weight'])[0] + _f64(sd['dense3.bias'])[0]
    return (q, r, ctx) if want_ctx else (q, r)


def actor_f64(actor, obs):
    """A ``ModelActorNetwork`` (or the reference's) -> ([logits [B,N,n] per head], next_state [B,N,D]), float64."""
    H, logits = ao.forward_f64(actor, obs)
    lin3 = actor.dense3.module
    return logits, H @ _f64(lin3.weight).T + _f64(lin3.bias)
