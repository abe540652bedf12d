"""CPU: the host side of the model-learning variant (rls/model/ac_network_model_multi_gumbel.py: an actor that also predicts the next
observation, an attention critic without the ReLU that also predicts the reward).

(a) tests/golden/model_forward.npz (made by tests/golden/make_model_golden.py from the REFERENCE's networks) holds the keys, shapes
    and size it should.
(b) tests/model_ref.py (float64 NumPy, written from the architecture) reproduces the reference's float64 outputs -- q, r, the policy
    logits and the predicted next observation -- to 1e-12: the same mathematics in another summation order.
(c) ``critic.ModelCriticNetwork`` / ``policy.ModelActorNetwork`` load the fixture state_dicts with ``strict=True`` and reproduce the
    reference's float32 q and r to 2e-6 (the bar of tests/test_critic_host.py), and its float64 actor outputs in float64 to 1e-12.
(d) ``pw_critic_forward_model`` is exported and refuses null / out-of-range arguments before anything is launched.
(e) ``fuse_model_attention`` with the two launches replaced by the float64 restatement (as tests/test_attention_host.py does).
"""
import copy
import ctypes as C
import os

import numpy as np
import pytest

from tests import attention_ref, lstm_ref
from tests import critic_ref as cr
from tests import model_ref as mr

torch = pytest.importorskip('torch')
nn = torch.nn

PATH = os.path.join(os.path.dirname(__file__), 'golden', mr.GOLDEN_FILE)
G = np.load(PATH)
CASES, ACTOR_CASES = mr.GOLDEN_CASES, mr.ACTOR_CASES
IDS, ACTOR_IDS = [cr.golden_name(*c) for c in CASES], [cr.golden_name(*c) for c in ACTOR_CASES]
CRITIC_KEYS = sorted(cr.KEYS + ('dense3.weight', 'dense3.bias'))


def fixture_state_dict(name, what='sd'):
    pre = '%s/%s/' % (name, what)
    return {k[len(pre):]: torch.from_numpy(G[k]) for k in G.files if k.startswith(pre)}


def _actor_keys(heads):
    lstm = ['bilstm.%s_l0%s' % (p, d) for d in ('', '_reverse') for p in ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh')]
    policy = ['dense2'] if len(heads) == 1 else ['dense2_1', 'dense2_2']
    return sorted(lstm + ['%s.module.%s' % (m, p) for m in ['dense1', 'dense3'] + policy for p in ('weight', 'bias')])


# ---- (a) ---------------------------------------------------------------------------------------------------------------------------
def test_fixture_holds_the_cases_and_the_reference_keys():
    for name in IDS:
        assert sorted(fixture_state_dict(name)) == CRITIC_KEYS
        for k, dt in (('q32', np.float32), ('q64', np.float64), ('r32', np.float32), ('r64', np.float64)):
            assert G['%s/%s' % (name, k)].shape == (cr.GOLDEN_ROWS, 1) and G['%s/%s' % (name, k)].dtype == dt
    for (N, D, heads), name in zip(ACTOR_CASES, ACTOR_IDS):
        assert sorted(fixture_state_dict(name, 'actor_sd')) == _actor_keys(heads)
        assert G[name + '/logits64'].shape == (cr.GOLDEN_ROWS, N, sum(heads)) and G[name + '/logits64'].dtype == np.float64
        assert G[name + '/next_state64'].shape == (cr.GOLDEN_ROWS, N, D) and G[name + '/next_state64'].dtype == np.float64
    assert [n for n in IDS if (n + '/logits64') in G.files] == ACTOR_IDS
    assert all(G[k].dtype.kind in 'fi' for k in G.files)     # arrays of numbers only
    assert os.path.getsize(PATH) < (1 << 20)


@pytest.mark.parametrize('N,D,heads', CASES, ids=IDS)
def test_inputs_are_the_rows_the_fixture_was_made_from(N, D, heads):
    obs, idx = cr.golden_inputs(N, D, heads)
    want = G[cr.golden_name(N, D, heads) + '/input_sum']
    assert obs.astype(np.float64).sum() == want[0] and float(idx.sum()) == want[1]


# ---- (b) ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,D,heads', CASES, ids=IDS)
def test_float64_restatement_reproduces_the_reference_critic(N, D, heads):
    name = cr.golden_name(N, D, heads)
    obs, idx = cr.golden_inputs(N, D, heads)
    q, r, ctx = mr.critic_f64(fixture_state_dict(name), obs, cr.one_hot(idx, heads), want_ctx=True)
    eq, er = float(np.abs(q - G[name + '/q64'][:, 0]).max()), float(np.abs(r - G[name + '/r64'][:, 0]).max())
    print('%s: |q_f64 - reference float64| %.3g, |r_f64 - reference float64| %.3g, min ctx %.3g' % (name, eq, er, ctx.min()))
    assert eq <= 1e-12 and er <= 1e-12
    assert ctx.min() < 0        # the fixture tells this critic from the ReLU form: a clamp would change q and r


def _actor(D, heads, dtype=torch.float32):
    from multiagent_rl_amd.policy import ModelActorNetwork
    return ModelActorNetwork(D, heads[0] if len(heads) == 1 else list(heads)).eval().to(dtype)


@pytest.mark.parametrize('N,D,heads', ACTOR_CASES, ids=ACTOR_IDS)
def test_float64_restatement_reproduces_the_reference_actor(N, D, heads):
    name = cr.golden_name(N, D, heads)
    actor = _actor(D, heads)
    actor.load_state_dict(fixture_state_dict(name, 'actor_sd'), strict=True)
    logits, nxt = mr.actor_f64(actor, cr.golden_inputs(N, D, heads)[0])
    el = float(np.abs(np.concatenate(logits, -1) - G[name + '/logits64']).max())
    en = float(np.abs(nxt - G[name + '/next_state64']).max())
    print('%s: |logits_f64 - reference| %.3g, |next_state_f64 - reference| %.3g' % (name, el, en))
    assert el <= 1e-12 and en <= 1e-12


# ---- (c) ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,D,heads', CASES, ids=IDS)
def test_model_critic_loads_reference_state_dict_and_reproduces_float32(N, D, heads):
    from multiagent_rl_amd.critic import ModelCriticNetwork
    name = cr.golden_name(N, D, heads)
    net = ModelCriticNetwork(D + sum(heads), 1).eval()
    sd = fixture_state_dict(name)
    assert {k: tuple(v.shape) for k, v in net.state_dict().items()} == {k: tuple(v.shape) for k, v in sd.items()}
    net.load_state_dict(sd, strict=True)
    obs, idx = cr.golden_inputs(N, D, heads)
    act = cr.one_hot(idx, heads)
    with torch.no_grad():
        out = net(torch.from_numpy(obs), torch.from_numpy(act))
        assert isinstance(out, tuple) and len(out) == 2
        q, r = (t.numpy() for t in out)
        if len(heads) == 2:   # a list of per-head one-hots is concatenated as the reference does
            parts = [torch.from_numpy(act[..., :heads[0]]), torch.from_numpy(act[..., heads[0]:])]
            assert np.array_equal(net(torch.from_numpy(obs), parts)[0].numpy(), q)
    assert q.shape == r.shape == (cr.GOLDEN_ROWS, 1)
    eq, er = float(np.abs(q - G[name + '/q32']).max()), float(np.abs(r - G[name + '/r32']).max())
    print('%s: |q - reference float32| %.3g, |r - reference float32| %.3g' % (name, eq, er))
    assert eq <= 2e-6 and er <= 2e-6


@pytest.mark.parametrize('N,D,heads', ACTOR_CASES, ids=ACTOR_IDS)
def test_model_actor_loads_reference_state_dict_and_reproduces_float64(N, D, heads):
    name = cr.golden_name(N, D, heads)
    actor = _actor(D, heads)
    sd = fixture_state_dict(name, 'actor_sd')
    assert {k: tuple(v.shape) for k, v in actor.state_dict().items()} == {k: tuple(v.shape) for k, v in sd.items()}
    actor.load_state_dict(sd, strict=True)
    with torch.no_grad():
        out = actor.double()(torch.from_numpy(cr.golden_inputs(N, D, heads)[0]).double())
    assert isinstance(out, tuple) and len(out) == 2
    policy, nxt = out
    logits = torch.cat(policy, -1) if isinstance(policy, list) else policy
    assert float(np.abs(logits.numpy() - G[name + '/logits64']).max()) <= 1e-12
    assert float(np.abs(nxt.numpy() - G[name + '/next_state64']).max()) <= 1e-12


def test_model_actor_with_two_heads_has_the_reference_keys():
    actor = _actor(21, (5, 10))
    assert sorted(actor.state_dict()) == _actor_keys((5, 10))
    policy, nxt = actor(torch.zeros(2, 3, 21))
    assert [tuple(p.shape) for p in policy] == [(2, 3, 5), (2, 3, 10)] and tuple(nxt.shape) == (2, 3, 21)


# ---- (d) ---------------------------------------------------------------------------------------------------------------------------
def test_critic_forward_model_arguments_are_checked_on_the_host():
    """PW_EINVAL with a text, nothing launched (no GPU needed; the pointers are fakes)."""
    from multiagent_rl_amd import _lib
    lib = _lib.load()
    assert 'pw_critic_forward_model' in _lib.SIGNATURES and hasattr(lib, 'pw_critic_forward_model')
    assert lib.pw_version() >= 115
    p = C.c_void_p(4096)
    w = [p] * 10

    def call(obs=p, idx=p, vec=None, n0=5, n1=0, weights=w, b=64, N=6, D=16, rew=None, done=None, q=p, r_pred=p, y=None):
        return lib.pw_critic_forward_model(obs, idx, vec, n0, n1, *weights, b, N, D, rew, done, 0.95, q, r_pred, y, None)

    def refused(text, **kw):
        assert call(**kw) == -1, kw
        assert text in lib.pw_last_error(), (kw, lib.pw_last_error())

    refused(b'null', obs=None)
    refused(b'null', q=None)
    refused(b'null', q=None, r_pred=None)
    for i in range(8):
        refused(b'null', weights=[None if j == i else p for j in range(10)])
        refused(b'null', weights=[None if j == i else p for j in range(10)], r_pred=None)
    refused(b'exactly one', idx=p, vec=p)
    refused(b'exactly one', idx=None, vec=None)
    refused(b'action widths', n0=0)
    refused(b'action widths', n1=-1)
    refused(b'action widths', n0=9, n1=8)
    refused(b'action widths', n0=17)
    refused(b'N must be', N=0)
    refused(b'N must be', N=65)
    refused(b'obs_dim', D=0)
    refused(b'obs_dim', D=105)
    refused(b'b must be', b=0)
    refused(b'TD target', y=p)
    refused(b'TD target', rew=p, y=p)
    refused(b'TD target', rew=p, done=p)
    refused(b'w3 and b3', weights=[p] * 8 + [None, p])
    refused(b'w3 and b3', weights=[p] * 8 + [p, None])
    refused(b'w3 and b3', weights=[p] * 8 + [None, None])


# ---- (e) ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def standins(monkeypatch):
    from multiagent_rl_amd import attention
    calls = []

    def fwd(Y, relu, keep):
        calls.append(('forward', bool(relu), keep))
        return attention_ref.launch_forward(Y, relu, keep)

    def bwd(dOut, Y, weight, out, relu):
        calls.append(('backward', bool(relu)))
        return attention_ref.launch_backward(dOut, Y, weight, out, relu)
    monkeypatch.setattr(attention, 'launch_forward', fwd)
    monkeypatch.setattr(attention, 'launch_backward', bwd)
    return calls


@pytest.fixture
def lstm_standins(monkeypatch):
    from multiagent_rl_amd import lstm
    monkeypatch.setattr(lstm, 'launch_forward', lstm_ref.launch_forward)
    monkeypatch.setattr(lstm, 'launch_backward', lstm_ref.launch_backward)
    return lstm


class _Wrap(nn.Module):
    def __init__(self, module):
        super().__init__()
        self.module = module

    def forward(self, x):
        return self.module(x)


class LookAlike(nn.Module):
    """A model critic of the same structure that is not the package's (the reference's own class in a user's checkout)."""

    def __init__(self, input_dim=15, width=1):
        super().__init__()
        self.dense1 = _Wrap(nn.Linear(input_dim, 64))
        self.lstm = nn.LSTM(64, 64, num_layers=1, batch_first=True)
        self.dense2 = nn.Linear(64, 1)
        self.dense3 = nn.Linear(64, width)

    def forward(self, obs, action):
        out = torch.relu(self.dense1(torch.cat([obs, action], dim=-1)))
        output, _ = self.lstm(out, None)
        ctx = attention_ref.stock(output, relu=False)
        return self.dense2(ctx), self.dense3(ctx)


def _model_critics():
    from multiagent_rl_amd.critic import ModelCriticNetwork
    torch.manual_seed(2)
    return [ModelCriticNetwork(15, 1), LookAlike()]


def test_fuse_model_attention_is_a_class_swap_and_round_trips(standins):
    from multiagent_rl_amd.attention import (FusedAttention, FusedModelAttention, fuse_attention, fuse_model_attention,
                                             unfuse_attention, unfuse_model_attention)
    from multiagent_rl_amd.critic import ModelCriticNetwork
    for net in _model_critics():
        cls = type(net)
        keys = list(net.state_dict().keys())
        params = [p.data_ptr() for p in net.parameters()]
        inputs = lstm_ref.network_inputs('critic', 4, 5, torch.float32)
        base = lstm_ref.network_grads(net, inputs)
        q0, r0 = (t.detach() for t in net(*inputs))
        assert fuse_attention(net) == 0 and type(net) is cls                 # the ReLU form's swap leaves it alone, as before
        assert fuse_model_attention(net) == 1 and fuse_model_attention(net) == 0
        assert fuse_attention(net) == 0 and unfuse_attention(net) == 0
        assert isinstance(net, FusedModelAttention) and not isinstance(net, FusedAttention)
        assert isinstance(net, cls) and type(net) is not cls
        assert list(net.state_dict().keys()) == keys and [p.data_ptr() for p in net.parameters()] == params
        del standins[:]
        got = lstm_ref.network_grads(net, inputs)                            # gradients reach every parameter, both heads included
        assert standins == [('forward', False, True), ('backward', False)]  # one launch each way, without the ReLU
        assert set(got) == set(base) and 'dense3.weight' in got
        for n in base:
            assert torch.allclose(got[n], base[n], rtol=1e-4, atol=1e-5), n
        out = net(*inputs)
        assert isinstance(out, tuple) and len(out) == 2
        assert torch.allclose(out[0], q0, atol=1e-5) and torch.allclose(out[1], r0, atol=1e-5)
        clone = copy.deepcopy(net)
        assert type(clone) is type(net)
        clone.load_state_dict((ModelCriticNetwork(15, 1) if cls is ModelCriticNetwork else cls()).state_dict())
        assert unfuse_model_attention(net) == 1 and type(net) is cls and unfuse_model_attention(net) == 0
        del standins[:]
        out = net(*inputs)
        assert torch.equal(out[0], q0) and torch.equal(out[1], r0) and standins == []    # the original forward again
        assert unfuse_model_attention(clone) == 1 and type(clone) is cls
    holder = nn.ModuleList(_model_critics() + [lstm_ref.make_network('critic')])          # found inside a container, each by its own swap
    assert fuse_model_attention(holder) == 2 and fuse_attention(holder) == 1
    assert unfuse_attention(holder) == 1 and unfuse_model_attention(holder) == 2
    assert fuse_model_attention(object()) == 0 and unfuse_model_attention(None) == 0


def test_fuse_model_attention_leaves_other_networks(standins):
    from multiagent_rl_amd.attention import fuse_model_attention
    from multiagent_rl_amd.policy import TimeDistributed
    for name in ('critic', 'bicnet', 'actor'):
        net = lstm_ref.make_network(name)
        cls = type(net)
        assert fuse_model_attention(net) == 0 and type(net) is cls
    wide = LookAlike(width=10)                                               # a dense3 of another width than dense2: some other network
    assert fuse_model_attention(wide) == 0 and type(wide) is LookAlike
    net = LookAlike()
    net.dense3 = TimeDistributed(nn.Linear(64, 1))
    assert fuse_model_attention(net) == 0
    net = LookAlike()
    net.lstm = nn.LSTM(64, 64, batch_first=True, bidirectional=True)
    assert fuse_model_attention(net) == 0


def test_long_agent_axis_and_handed_back_go_to_the_original_forward(standins, monkeypatch):
    from multiagent_rl_amd import attention
    net = _model_critics()[0]
    assert attention.fuse_model_attention(net) == 1
    obs, act = torch.randn(2, 65, 10), torch.randn(2, 65, 5)
    q, r = net(obs, act)
    assert standins == [] and q.shape == r.shape == (2, 1)
    monkeypatch.setattr(attention, 'HANDED_BACK', (5,))
    net(*lstm_ref.network_inputs('critic', 4, 5, torch.float32))
    assert standins == []
    net(*lstm_ref.network_inputs('critic', 4, 6, torch.float32))
    assert [c[0] for c in standins] == ['forward']


@pytest.mark.parametrize('order', ['attention first', 'lstm first'])
def test_fuse_lstm_composes_in_either_order(standins, lstm_standins, order):
    from multiagent_rl_amd.attention import fuse_model_attention, unfuse_model_attention
    net = _model_critics()[0]
    inputs = lstm_ref.network_inputs('critic', 4, 5, torch.float32)
    base = lstm_ref.network_grads(net, inputs)
    steps = [fuse_model_attention, lstm_standins.fuse_lstm]
    for f in (steps if order == 'attention first' else steps[::-1]):
        assert f(net) == 1
    assert type(net.lstm) is lstm_standins.FusedLSTM
    got = lstm_ref.network_grads(net, inputs)
    assert ('forward', False, True) in standins and ('backward', False) in standins
    for n in base:
        assert torch.allclose(got[n], base[n], rtol=1e-4, atol=1e-5), n
    assert unfuse_model_attention(net) == 1 and lstm_standins.unfuse_lstm(net) == 1
    assert type(net.lstm) is nn.LSTM


def test_fuse_trainer_routes_a_model_critic_to_the_model_swap(standins):
    from multiagent_rl_amd.attention import FusedAttention, FusedModelAttention, fuse_trainer

    class T(object):
        pass
    t = T()
    t.critic, t.target_critic = _model_critics()[0], lstm_ref.make_network('critic')
    assert fuse_trainer(t) == 2
    assert isinstance(t.critic, FusedModelAttention) and isinstance(t.target_critic, FusedAttention)
