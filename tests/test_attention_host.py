"""CPU: the host side of pw_attention_pool_forward / pw_attention_pool_backward and of multiagent_rl_amd.attention (no launch happens
without a GPU: every call into the library here is refused before one), the float64 restatement tests/attention_ref.py against float64
autograd of the stock expression, and the Python plumbing (autograd function, fuse_attention) with the two launches replaced by that
restatement.

Bound.  Restatement in float64 against autograd in float64: 1e-12 (the same mathematics; what differs is the summation order of dot
products of 64 terms and sums over at most 7 steps of numbers below 1: a few 1e-15)."""
import copy
import inspect
import os
import re
import sys

import pytest

from multiagent_rl_amd import _lib
from tests import attention_ref, lstm_ref

torch = pytest.importorskip('torch')
nn = torch.nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


# ---- the restatement --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('relu', [True, False], ids=['relu', 'linear'])
@pytest.mark.parametrize('b,N', [(3, 1), (4, 2), (5, 7)])
def test_restatement_equals_float64_autograd(b, N, relu):
    Y, dOut = attention_ref.make_inputs(b, N, torch.float64)
    ref = attention_ref.grads(lambda y: attention_ref.stock(y, relu), Y, lambda o: (o * dOut).sum())
    out, w = attention_ref.forward(Y, relu)
    dY = attention_ref.backward(dOut, Y, w, out, relu)
    assert float(w.sum(dim=1).sub(1).abs().max()) <= 1e-12
    assert float((out - ref['out']).abs().max()) <= 1e-12 and float((dY - ref['dY']).abs().max()) <= 1e-12
    assert float(ref['dY'].abs().max()) > 0


# ---- the plumbing, with stand-ins for the two launches ----------------------------------------------------------------------------
@pytest.fixture
def standins(monkeypatch):
    from multiagent_rl_amd import attention
    calls = []

    def fwd(Y, relu, keep):
        calls.append(('forward', keep))
        return attention_ref.launch_forward(Y, relu, keep)

    def bwd(dOut, Y, weight, out, relu):
        calls.append(('backward', dOut.is_contiguous()))
        return attention_ref.launch_backward(dOut, Y, weight, out, relu)
    monkeypatch.setattr(attention, 'launch_forward', fwd)
    monkeypatch.setattr(attention, 'launch_backward', bwd)
    attention.calls = calls
    yield attention
    del attention.calls


@pytest.fixture
def lstm_standins(monkeypatch):
    from multiagent_rl_amd import lstm
    monkeypatch.setattr(lstm, 'launch_forward', lstm_ref.launch_forward)
    monkeypatch.setattr(lstm, 'launch_backward', lstm_ref.launch_backward)
    return lstm


@pytest.mark.parametrize('relu', [True, False], ids=['relu', 'linear'])
def test_attention_pool_function(standins, relu):
    """Gradients flow and equal autograd of the stock expression; nothing is saved without a gradient; an expanded dOut arrives
    contiguous."""
    Y, dOut = attention_ref.make_inputs(5, 7, torch.float64)
    want = attention_ref.grads(lambda y: attention_ref.stock(y, relu), Y, lambda o: (o * dOut).sum())
    got = attention_ref.grads(lambda y: standins.attention_pool(y, relu), Y, lambda o: (o * dOut).sum())
    assert float((got['out'] - want['out']).abs().max()) <= 1e-12 and float((got['dY'] - want['dY']).abs().max()) <= 1e-12
    assert standins.calls == [('forward', True), ('backward', True)]
    del standins.calls[:]
    want = attention_ref.grads(lambda y: attention_ref.stock(y, relu), Y, lambda o: o.sum())
    got = attention_ref.grads(lambda y: standins.attention_pool(y, relu), Y, lambda o: o.sum())    # out.sum(): an expanded zero-stride dOut
    assert float((got['dY'] - want['dY']).abs().max()) <= 1e-12 and standins.calls == [('forward', True), ('backward', True)]
    del standins.calls[:]
    Yg = Y.clone().requires_grad_(True)
    with torch.no_grad():
        out = standins.attention_pool(Yg, relu)
    assert not out.requires_grad and out.grad_fn is None
    out = standins.attention_pool(Y, relu)                                                          # an input that needs no gradient
    assert not out.requires_grad
    assert standins.calls == [('forward', False), ('forward', False)]
    out = standins.attention_pool(Yg.transpose(0, 1).contiguous().transpose(0, 1), relu)            # a strided Y is made contiguous
    out.sum().backward()
    assert float((Yg.grad - want['dY']).abs().max()) <= 1e-12


def test_attention_pool_refusals():
    from multiagent_rl_amd import attention
    with pytest.raises(RuntimeError, match='no CPU fallback'):     # the real launch function is in place
        attention.attention_pool(torch.zeros(2, 3, 64))
    with pytest.raises(ValueError, match=r'\[b, N, 64\]'):
        attention.attention_pool(torch.zeros(2, 3, 32))
    with pytest.raises(ValueError, match=r'\[b, N, 64\]'):
        attention.attention_pool(torch.zeros(3, 64))
    with pytest.raises(ValueError, match='steps'):
        attention.attention_pool(torch.zeros(2, 65, 64))
    with pytest.raises(ValueError, match='steps'):
        attention.attention_pool(torch.zeros(2, 0, 64))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        attention.launch_backward(torch.zeros(2, 64), torch.zeros(2, 3, 64), torch.zeros(2, 3), torch.zeros(2, 64), True)


class _Wrap(nn.Module):
    def __init__(self, module):
        super().__init__()
        self.module = module

    def forward(self, x):
        return self.module(x)


class LookAlike(nn.Module):
    """A critic of the same structure that is not the package's (the reference's own class in a user's checkout)."""

    def __init__(self, input_dim=15):
        super().__init__()
        self.dense1 = _Wrap(nn.Linear(input_dim, 64))
        self.lstm = nn.LSTM(64, 64, num_layers=1, batch_first=True)
        self.dense2 = nn.Linear(64, 1)

    def forward(self, obs, action):
        out = torch.relu(self.dense1(torch.cat([obs, action], dim=-1)))
        output, (h, _) = self.lstm(out, None)
        return self.dense2(torch.relu(attention_ref.stock(output, relu=False)))


class WithThirdHead(LookAlike):
    """The model-learning variant's shape: a second head and no ReLU."""

    def __init__(self):
        super().__init__()
        self.dense3 = nn.Linear(64, 10)


def _critics():
    torch.manual_seed(2)
    return [lstm_ref.make_network('critic'), LookAlike()]


def test_fuse_attention_is_a_class_swap_and_round_trips(standins):
    from multiagent_rl_amd.attention import FusedAttention, fuse_attention, unfuse_attention
    from multiagent_rl_amd.critic import CriticNetwork
    for net in _critics():
        cls = type(net)
        keys = list(net.state_dict().keys())
        params = [p.data_ptr() for p in net.parameters()]
        inputs = lstm_ref.network_inputs('critic', 4, 5, torch.float32)
        base = lstm_ref.network_grads(net, inputs)
        q0 = net(*inputs).detach()
        assert fuse_attention(net) == 1 and fuse_attention(net) == 0
        assert isinstance(net, FusedAttention) and isinstance(net, cls) and type(net) is not cls
        assert list(net.state_dict().keys()) == keys and [p.data_ptr() for p in net.parameters()] == params
        del standins.calls[:]
        got = lstm_ref.network_grads(net, inputs)                            # gradients flow through the stand-ins to every parameter
        assert standins.calls == [('forward', True), ('backward', True)]
        assert set(got) == set(base)
        for n in base:
            assert torch.allclose(got[n], base[n], rtol=1e-4, atol=1e-5), n
        assert torch.allclose(net(*inputs), q0, atol=1e-5)
        clone = copy.deepcopy(net)
        assert type(clone) is type(net) and isinstance(clone, FusedAttention)
        fresh = CriticNetwork(15, 1) if cls is CriticNetwork else cls()
        clone.load_state_dict(fresh.state_dict())                            # a stock network's file loads unchanged
        assert unfuse_attention(net) == 1 and type(net) is cls and unfuse_attention(net) == 0
        del standins.calls[:]
        assert torch.equal(net(*inputs), q0) and standins.calls == []       # the original forward again
        assert unfuse_attention(clone) == 1 and type(clone) is cls
    holder = nn.ModuleList(_critics())                                       # critics inside a container are found
    assert fuse_attention(holder) == 2 and unfuse_attention(holder) == 2
    assert fuse_attention(object()) == 0 and unfuse_attention(None) == 0


def test_fuse_attention_leaves_what_has_no_such_block(standins):
    from multiagent_rl_amd.attention import fuse_attention
    from multiagent_rl_amd.critic import BiCNetCritic
    from multiagent_rl_amd.policy import TimeDistributed
    bic, third = lstm_ref.make_network('bicnet'), WithThirdHead()
    assert fuse_attention(bic) == 0 and type(bic) is BiCNetCritic
    assert fuse_attention(third) == 0 and type(third) is WithThirdHead
    assert fuse_attention(lstm_ref.make_network('actor')) == 0
    for change in ('hidden', 'layers', 'bidirectional', 'batch_first', 'dense1', 'dense2'):
        net = lstm_ref.make_network('critic')
        if change == 'hidden':
            net.lstm = nn.LSTM(64, 32, batch_first=True)
        elif change == 'layers':
            net.lstm = nn.LSTM(64, 64, num_layers=2, batch_first=True)
        elif change == 'bidirectional':
            net.lstm = nn.LSTM(64, 64, batch_first=True, bidirectional=True)
        elif change == 'batch_first':
            net.lstm = nn.LSTM(64, 64)
        elif change == 'dense1':
            net.dense1 = nn.Linear(15, 64)
        else:
            net.dense2 = TimeDistributed(nn.Linear(64, 1))
        assert fuse_attention(net) == 0, change


def test_an_agent_axis_beyond_the_bound_takes_the_stock_path(standins, monkeypatch):
    from multiagent_rl_amd.attention import fuse_attention
    net = lstm_ref.make_network('critic')
    stock = copy.deepcopy(net)
    assert fuse_attention(net) == 1
    for N in (65, 80):
        inputs = lstm_ref.network_inputs('critic', 2, N, torch.float32)
        want, got = lstm_ref.network_grads(stock, inputs), lstm_ref.network_grads(net, inputs)
        assert standins.calls == [] and all(torch.equal(got[n], want[n]) for n in want)
    inputs = lstm_ref.network_inputs('critic', 2, 64, torch.float32)
    net(*inputs)
    assert standins.calls == [('forward', True)]
    del standins.calls[:]
    monkeypatch.setattr(standins, 'HANDED_BACK', (6,))                       # a length listed as handed back goes the same way
    inputs = lstm_ref.network_inputs('critic', 2, 6, torch.float32)
    assert torch.equal(net(*inputs), stock(*inputs)) and standins.calls == []


@pytest.mark.parametrize('order', ['attention first', 'lstm first'])
def test_composes_with_fuse_lstm(standins, lstm_standins, order):
    from multiagent_rl_amd.attention import FusedAttention, fuse_attention, unfuse_attention
    from multiagent_rl_amd.lstm import FusedLSTM, fuse_lstm
    stock = lstm_ref.make_network('critic')
    net, ref = copy.deepcopy(stock), copy.deepcopy(stock).double()
    steps = (fuse_attention, fuse_lstm) if order == 'attention first' else (fuse_lstm, fuse_attention)
    assert [f(net) for f in steps] == [1, 1]
    assert isinstance(net, FusedAttention) and type(net.lstm) is FusedLSTM
    inputs = lstm_ref.network_inputs('critic', 33, 6, torch.float32)
    g_ref = lstm_ref.network_grads(ref, tuple(t.double() for t in inputs))
    ratio, worst, e_k, e_s = lstm_ref.worst_ratio(lstm_ref.network_grads(net, inputs), lstm_ref.network_grads(stock, inputs), g_ref)
    assert standins.calls == [('forward', True), ('backward', True)]
    assert ratio <= 4.0, (worst, e_k, e_s)
    assert unfuse_attention(net) == 1 and type(net) is type(stock) and type(net.lstm) is FusedLSTM


def test_trainer_switches_are_off_by_default_and_take_both_critics(standins):
    from multiagent_rl_amd.attention import FusedAttention, fuse_trainer
    from multiagent_rl_amd.policy import accelerate_trainer

    class T(object):
        pass
    t = T()
    t.actor, t.critic = lstm_ref.make_network('actor'), lstm_ref.make_network('critic')
    t.target_actor, t.target_critic = copy.deepcopy(t.actor), copy.deepcopy(t.critic)
    assert fuse_trainer(t) == 2 and isinstance(t.critic, FusedAttention) and isinstance(t.target_critic, FusedAttention)
    t.critic, t.target_critic = lstm_ref.make_network('critic'), object()    # a wrapped target network is left alone
    assert fuse_trainer(t) == 1
    assert inspect.signature(accelerate_trainer).parameters['attention'].default is False
    sys.path.insert(0, os.path.join(ROOT, 'examples'))
    try:
        import madr_learner
        import train_batched
    finally:
        sys.path.pop(0)
    assert inspect.signature(madr_learner.Trainer.__init__).parameters['fused_attention'].default is False
    with pytest.raises(SystemExit):                                          # refused like --fused-targets without an attention critic
        train_batched.main(['--fused-attention'])
    with pytest.raises(SystemExit):
        train_batched.main(['--fused-attention', '--critic', 'bicnet'])


# ---- the C entry points -----------------------------------------------------------------------------------------------------------
P = [4096 + 1024 * k for k in range(6)]    # fake, 4-byte aligned "device pointers": every call below is refused before a launch


def _fwd(Y=P[0], b=8, N=6, H=64, relu=1, out=P[1], weight=P[2]):
    return _lib.load().pw_attention_pool_forward(Y, b, N, H, relu, out, weight, None)


def _bwd(dOut=P[3], Y=P[0], weight=P[2], out=P[1], b=8, N=6, H=64, relu=1, dY=P[4]):
    return _lib.load().pw_attention_pool_backward(dOut, Y, weight, out, b, N, H, relu, dY, None)


def test_symbols_are_exported_and_declared():
    lib = _lib.load()
    header = open(os.path.join(ROOT, 'include', 'pworld.h')).read()
    for name in ('pw_attention_pool_forward', 'pw_attention_pool_backward'):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
        assert re.search(r'\bint %s\(' % name, header)
    assert lib.pw_version() >= 114


@pytest.mark.parametrize('call', [_fwd, _bwd], ids=['forward', 'backward'])
@pytest.mark.parametrize('kw,word', [
    (dict(H=32), b'H'), (dict(H=128), b'H'), (dict(H=0), b'H'), (dict(H=-64), b'H'),
    (dict(N=0), b'N must'), (dict(N=-1), b'N must'), (dict(N=65), b'N must'), (dict(N=1 << 20), b'N must'),
    (dict(b=0), b'b must'), (dict(b=-4), b'b must'), (dict(b=1 << 40), b'b:'),
    (dict(Y=None), b'Y is null'), (dict(Y=P[0] + 2), b'Y must be 4-byte aligned'),
    (dict(out=None), b'out is null'), (dict(out=P[1] + 1), b'out must be 4-byte aligned'),
    (dict(weight=P[2] + 3), b'weight must be 4-byte aligned'),
], ids=lambda v: str(v) if isinstance(v, dict) else '')
def test_both_entry_points_refuse_bad_shared_arguments(call, kw, word):
    assert call(**kw) == EINVAL
    assert word in _lib.load().pw_last_error(), _lib.load().pw_last_error()


def test_backward_refuses_bad_buffers():
    lib = _lib.load()
    for name in ('dOut', 'weight', 'dY'):
        assert _bwd(**{name: None}) == EINVAL and name.encode() + b' is null' in lib.pw_last_error()
    for name in ('dOut', 'dY'):
        assert _bwd(**{name: P[5] + 2}) == EINVAL and name.encode() + b' must be 4-byte aligned' in lib.pw_last_error()


# ---- what the compiler made of the new unit ---------------------------------------------------------------------------------------
def test_attention_unit_carries_exactly_its_own_kernels():
    """Mirrors test_lstm_unit_carries_exactly_its_own_kernels: the unit includes pw_lstm_math.hpp / pw_common.hpp for their device
    functions and must not pick up a kernel with them."""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    try:
        import code_object
    finally:
        sys.path.pop(0)
    if not code_object.tools_present():
        pytest.skip('ROCm LLVM binary tools not installed')
    from multiagent_rl_amd import build_native
    if not all(os.path.exists(o) for o in build_native.objects()):
        build_native.build(force=True)
    src = open(os.path.join(ROOT, 'multiagent_rl_amd', 'csrc', 'pw_kernels_attention.hpp')).read()
    defined = set(re.findall(r'__global__ void (?:__launch_bounds__\(\w+\) )?(pw_\w+_kernel)\(', src))
    assert defined == {'pw_attention_pool_forward_kernel', 'pw_attention_pool_backward_kernel'}
    names = code_object.per_unit_kernels()['pworld_attention']
    assert len(names) == 2 and {re.match(r'(?:void )?(\w+)', n).group(1) for n in names} == defined
    assert os.path.join(build_native.HERE, 'csrc', 'pworld_attention.hip') in build_native.SRCS
    assert 'pworld_attention' in build_native.unit_sources.__doc__
