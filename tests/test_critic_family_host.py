"""CPU: what the three critic modules (CriticNetwork, BiCNetCritic, ModelCriticNetwork) share -- the base ``__init__``, the trunk
(``attention.lstm_trunk``), the attention expression (``attention.attend``) and the structural classifier (``attention.critic_form``).

(a) ``state_dict`` keys are the reference's, in its order, and seeded construction draws the parameters in the order dense1, lstm,
    dense2, dense3 (bitwise against stock layers built inline under the same seed).
(b) ``forward`` and the parameter gradients of ``out.sum()`` are bitwise those of the reference's expression written inline on the
    net's own submodules (query ``h_n[-1]``; ReLU for the attention critic, none for the model critic).
(c) The classifier as a table, and who is left alone by the swaps and refused by ``FusedCritic``.
"""
import pytest

torch = pytest.importorskip('torch')
import torch.nn as nn  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from multiagent_rl_amd import _lib  # noqa: E402
from multiagent_rl_amd.attention import critic_form, fuse_attention, fuse_model_attention, fuse_trainer  # noqa: E402
from multiagent_rl_amd.critic import BiCNetCritic, CriticNetwork, FusedCritic, ModelCriticNetwork  # noqa: E402
from multiagent_rl_amd.policy import ActorNetwork, TimeDistributed  # noqa: E402

D, A = 10, 5
TRUNK_KEYS = ['dense1.module.weight', 'dense1.module.bias', 'lstm.weight_ih_l0', 'lstm.weight_hh_l0', 'lstm.bias_ih_l0', 'lstm.bias_hh_l0']
KEYS = {CriticNetwork: TRUNK_KEYS + ['dense2.weight', 'dense2.bias'],
        BiCNetCritic: TRUNK_KEYS + ['dense2.module.weight', 'dense2.module.bias'],
        ModelCriticNetwork: TRUNK_KEYS + ['dense2.weight', 'dense2.bias', 'dense3.weight', 'dense3.bias']}
CLASSES = [CriticNetwork, BiCNetCritic, ModelCriticNetwork]


@pytest.mark.parametrize('cls', CLASSES, ids=lambda c: c.__name__)
def test_keys_and_seeded_construction_order(cls):
    assert list(cls(D + A, 1).state_dict().keys()) == KEYS[cls]
    for seed in (0, 7):
        torch.manual_seed(seed)
        net = cls(D + A, 1)
        torch.manual_seed(seed)
        stock = [TimeDistributed(nn.Linear(D + A, 64)), nn.LSTM(64, 64, num_layers=1, batch_first=True, bidirectional=False),
                 nn.Linear(64, 1), nn.Linear(64, 1)]
        want = [p for layer in stock for p in layer.state_dict().values()][:len(KEYS[cls])]
        got = list(net.state_dict().values())
        assert len(got) == len(want) and all(torch.equal(g, w) for g, w in zip(got, want)), (cls.__name__, seed)


def _inline(net, obs, action):
    """The reference's forward, written out on ``net``'s own submodules."""
    parts = [obs] + (list(action) if isinstance(action, (list, tuple)) else [action])
    hid = F.relu(net.dense1(torch.cat(parts, dim=-1)))
    steps, (h_n, _) = net.lstm(hid, None)
    if isinstance(net, BiCNetCritic):
        return net.dense2(steps)
    score = torch.bmm(steps, h_n[-1].unsqueeze(2)).squeeze(2)
    weight = F.softmax(score, dim=1)
    ctx = torch.bmm(steps.transpose(1, 2), weight.unsqueeze(2)).squeeze(2)
    if isinstance(net, ModelCriticNetwork):
        return net.dense2(ctx), net.dense3(ctx)
    return net.dense2(F.relu(ctx))


def _grads(net, out):
    net.zero_grad()
    sum(o.sum() for o in out).backward() if isinstance(out, tuple) else out.sum().backward()
    return [p.grad.clone() for p in net.parameters()]


@pytest.mark.parametrize('as_list', [False, True], ids=['tensor', 'list'])
@pytest.mark.parametrize('N', [1, 4])
@pytest.mark.parametrize('cls', CLASSES, ids=lambda c: c.__name__)
def test_forward_and_gradients_are_bitwise_the_inline_expression(cls, N, as_list):
    torch.manual_seed(100 + N)
    net = cls(D + A, 1)
    obs, act = torch.randn(3, N, D), torch.randn(3, N, A)
    action = [act[..., :2], act[..., 2:]] if as_list else act
    got, want = net(obs, action), _inline(net, obs, action)
    if cls is ModelCriticNetwork:
        assert isinstance(got, tuple) and len(got) == 2 and all(torch.equal(g, w) for g, w in zip(got, want))
        assert got[0].shape == (3, 1) and got[1].shape == (3, 1)
    else:
        assert got.shape == ((3, N, 1) if cls is BiCNetCritic else (3, 1)) and torch.equal(got, want)
    g_got, g_want = _grads(net, got), _grads(net, want)
    assert all(torch.equal(a, b) for a, b in zip(g_got, g_want))
    assert any(float(g.abs().max()) > 0 for g in g_got)


def _with(net, **layers):
    for name, layer in layers.items():
        setattr(net, name, layer)
    return net


def _not_critics():
    return {
        'actor': ActorNetwork(D, A),
        'bidirectional lstm': _with(CriticNetwork(D + A), lstm=nn.LSTM(64, 64, batch_first=True, bidirectional=True)),
        'hidden size 32': _with(CriticNetwork(D + A), lstm=nn.LSTM(64, 32, batch_first=True)),
        'two layers': _with(CriticNetwork(D + A), lstm=nn.LSTM(64, 64, num_layers=2, batch_first=True)),
        'per-step dense3': _with(ModelCriticNetwork(D + A), dense3=TimeDistributed(nn.Linear(64, 1))),
        'dense3 beside a per-step dense2': _with(BiCNetCritic(D + A), dense3=nn.Linear(64, 1)),
    }


def test_classifier_table():
    assert critic_form(CriticNetwork(D + A)) == ('attention', (1,))
    assert critic_form(BiCNetCritic(D + A)) == ('steps', (1,))
    assert critic_form(ModelCriticNetwork(D + A)) == ('model', (1, 1))
    assert critic_form(CriticNetwork(D + A, 3)) == ('attention', (3,))          # the widths found, whatever they are
    assert critic_form(ModelCriticNetwork(D + A, 2)) == ('model', (2, 2))
    for what, net in _not_critics().items():
        assert critic_form(net) == (None, ()), what
        assert fuse_attention(net) == 0 and fuse_model_attention(net) == 0, what


def test_a_dense3_of_another_width_is_served_by_neither_swap():
    net = _with(ModelCriticNetwork(D + A), dense3=nn.Linear(64, 2))
    cls = type(net)
    assert critic_form(net)[0] is None
    assert fuse_attention(net) == 0 and fuse_model_attention(net) == 0 and type(net) is cls

    class _T(object):
        critic = target_critic = net
    assert fuse_trainer(_T()) == 0 and type(net) is cls


def test_fused_critic_refuses_what_the_kernels_do_not_serve(monkeypatch):
    """The constructor classifies before it touches the parameters, so this needs neither the library nor a GPU."""
    monkeypatch.setattr(_lib, 'load', lambda: None)
    refused = dict(_not_critics(), **{'model critic of width 2': ModelCriticNetwork(D + A, 2), 'attention critic of width 2': CriticNetwork(D + A, 2),
                                      'dense3 of another width': _with(ModelCriticNetwork(D + A), dense3=nn.Linear(64, 2))})
    for what, net in refused.items():
        with pytest.raises(ValueError, match='FusedCritic serves'):
            FusedCritic(net)
    for cls in CLASSES:
        with pytest.raises(RuntimeError, match='needs the critic on the GPU'):   # classified and accepted; then the CPU parameters
            FusedCritic(cls(D + A))
