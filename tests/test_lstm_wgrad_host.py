"""CPU: the Python side of the W_hh gradient switch (multiagent_rl_amd.lstm: launch_wgrad, lstm_recurrence(wgrad=True),
fuse_lstm(wgrad=True), accelerate_trainer(wgrad=True), the example learner's fused_wgrad) with all three launches replaced by float64
restatements (tests/lstm_ref.py, tests/lstm_wgrad_ref.py), and the host side of pw_lstm_train_wgrad (every call into the library here
is refused before a launch).

Bound of the float64 comparison: 1e-12, tests/test_lstm_host.py's for the same mathematics in another summation order."""
import copy
import inspect
import os
import re
import sys

import pytest

from multiagent_rl_amd import _lib
from tests import lstm_ref, lstm_wgrad_ref

torch = pytest.importorskip('torch')
nn = torch.nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


@pytest.fixture
def standins(monkeypatch):
    """multiagent_rl_amd.lstm with the three launches replaced; ``calls`` lists the (want_fw, want_bw) of every launch_wgrad."""
    from multiagent_rl_amd import lstm
    calls = []

    def wgrad(dG, Y, want_fw, want_bw):
        calls.append((bool(want_fw), bool(want_bw)))
        return lstm_wgrad_ref.launch_wgrad(dG, Y, want_fw, want_bw)
    monkeypatch.setattr(lstm, 'launch_forward', lstm_ref.launch_forward)
    monkeypatch.setattr(lstm, 'launch_backward', lstm_ref.launch_backward)
    monkeypatch.setattr(lstm, 'launch_wgrad', wgrad)
    lstm.calls = calls
    yield lstm
    del lstm.calls


def _pieces(dirs, H, b, N):
    lstm = lstm_ref.make_lstm(dirs, H, torch.float64)
    w_ih, bias, w_fw, w_bw = [None if t is None else t.detach().clone() for t in lstm_ref.projection(lstm)]
    x, dY = lstm_ref.make_inputs(b, N, dirs, H, torch.float64)
    G = torch.nn.functional.linear(x, w_ih, bias).view(b, N, dirs, 4 * H)
    return lstm, x, dY, G, [w for w in (w_fw, w_bw) if w is not None]


@pytest.mark.parametrize('b,N,dirs,H', lstm_ref.SHAPES)
def test_recurrence_with_the_switch_equals_float64_autograd_of_the_stock_lstm(standins, b, N, dirs, H):
    lstm, x, dY, G, ws = _pieces(dirs, H, b, N)
    G = G.clone().requires_grad_(True)
    ws = [w.requires_grad_(True) for w in ws]
    Y = standins.lstm_recurrence(G, *ws, wgrad=True)
    grads = torch.autograd.grad(Y, [G] + ws, dY)
    assert standins.calls == [(True, dirs == 2)]                           # exactly one call per backward
    want = lstm_ref.autograd_grads(lstm, x, dY)                            # float64 autograd through nn.LSTM
    assert float((Y.detach() - want['Y']).abs().max()) <= 1e-12
    for g, key in zip(grads[1:], ('weight_hh_l0', 'weight_hh_l0_reverse')):
        assert g.shape == (4 * H, H)
        assert float((g - want[key]).abs().max()) <= 1e-12, key
        assert N > 1 or float(g.abs().max()) == 0.0                        # N = 1: zeros
    # dG reaches x through the projection: the input gradient of the stock LSTM
    w_ih = lstm_ref.projection(lstm)[0].detach()
    assert float(((grads[0].reshape(b * N, -1) @ w_ih).view_as(x) - want['x']).abs().max()) <= 1e-12


@pytest.mark.parametrize('dirs,H', [(1, 64), (2, 32)])
def test_gradcheck_with_the_switch(standins, dirs, H):
    _, _, _, G, ws = _pieces(dirs, H, 2, 3)
    # once_differentiable: first order only; the function is deterministic in float64
    leaves = [G.clone().requires_grad_(True)] + [w.clone().requires_grad_(True) for w in ws]
    assert torch.autograd.gradcheck(lambda g, *w: standins.lstm_recurrence(g, *w, wgrad=True), leaves, eps=1e-6, atol=1e-6, rtol=1e-5,
                                    fast_mode=True)


def test_launch_wgrad_is_called_for_the_directions_that_need_a_gradient(standins):
    _, _, dY, G, ws = _pieces(2, 32, 3, 4)
    want_fw, want_bw = lstm_wgrad_ref.whh_grads(*_dG_and_Y(G, ws, dY))

    def run(need_G, need_fw, need_bw):
        del standins.calls[:]
        leaves = [G.clone().requires_grad_(need_G), ws[0].clone().requires_grad_(need_fw), ws[1].clone().requires_grad_(need_bw)]
        Y = standins.lstm_recurrence(*leaves, wgrad=True)
        Y.backward(dY)
        return leaves
    g, fw, bw = run(True, True, False)
    assert standins.calls == [(True, False)] and bw.grad is None and float((fw.grad - want_fw).abs().max()) <= 1e-12
    g, fw, bw = run(False, False, True)
    assert standins.calls == [(False, True)] and fw.grad is None and float((bw.grad - want_bw).abs().max()) <= 1e-12
    g, fw, bw = run(True, False, False)
    assert standins.calls == [] and g.grad is not None and fw.grad is None and bw.grad is None     # not called at all
    run(True, True, True)
    assert standins.calls == [(True, True)]


def _dG_and_Y(G, ws, dY):
    Y, saved = lstm_ref.forward(G, *ws)
    return lstm_ref.backward(dY, saved, *ws), Y


def test_the_switch_off_never_calls_launch_wgrad(standins):
    for dirs, H in ((1, 64), (2, 32)):
        _, _, dY, G, ws = _pieces(dirs, H, 3, 4)
        leaves = [G.clone().requires_grad_(True)] + [w.clone().requires_grad_(True) for w in ws]
        for kw in ({}, {'wgrad': False}):
            standins.lstm_recurrence(*leaves, **kw).backward(dY)
        net = lstm_ref.make_network('critic' if dirs == 1 else 'actor')
        assert standins.fuse_lstm(net) == 1
        lstm_ref.network_grads(net, lstm_ref.network_inputs('critic' if dirs == 1 else 'actor', 3, 4, torch.float32))
    assert standins.calls == []
    assert inspect.signature(standins.lstm_recurrence).parameters['wgrad'].default is False
    assert inspect.signature(standins.fuse_lstm).parameters['wgrad'].default is False


def test_handed_back_lengths_take_the_gemm_path(standins, monkeypatch):
    assert set(standins.WGRAD_HANDED_BACK) == {(1, 64), (2, 32)}
    monkeypatch.setitem(standins.WGRAD_HANDED_BACK, (1, 64), (4,))
    _, _, dY, G, ws = _pieces(1, 64, 3, 4)
    leaves = [G.clone().requires_grad_(True), ws[0].clone().requires_grad_(True)]
    standins.lstm_recurrence(*leaves, wgrad=True).backward(dY)
    assert standins.calls == []
    assert float((leaves[1].grad - lstm_wgrad_ref.whh_grads(*_dG_and_Y(G, ws, dY))[0]).abs().max()) <= 1e-12


@pytest.mark.parametrize('b,N', [(33, 6), (4, 1)])
@pytest.mark.parametrize('name', lstm_ref.NETWORKS)
def test_fused_networks_with_the_switch_against_float64(standins, name, b, N):
    stock = lstm_ref.make_network(name)
    fused, ref = copy.deepcopy(stock), copy.deepcopy(stock).double()
    assert standins.fuse_lstm(fused, wgrad=True) == 1
    inputs = lstm_ref.network_inputs(name, b, N, torch.float32)
    g_ref = lstm_ref.network_grads(ref, tuple(t.double() for t in inputs))
    g_stock, g_fused = lstm_ref.network_grads(stock, inputs), lstm_ref.network_grads(fused, inputs)
    assert len(standins.calls) == 1
    ratio, worst, e_k, e_s = lstm_ref.worst_ratio(g_fused, g_stock, g_ref)
    print('%s b=%d N=%d: worst %s fused %.3e stock %.3e ratio %.2f' % (name, b, N, worst, e_k, e_s, ratio))
    assert set(g_fused) == set(g_ref) and ratio <= 4.0, (worst, e_k, e_s)


def test_the_mode_is_an_instance_attribute_of_the_swapped_lstm():
    from multiagent_rl_amd.lstm import FusedLSTM, fuse_lstm, unfuse_lstm
    for name in lstm_ref.NETWORKS:
        net = lstm_ref.make_network(name)
        keys = list(net.state_dict().keys())
        rnn = [m for m in net.modules() if isinstance(m, nn.LSTM)][0]
        assert fuse_lstm(net, wgrad=True) == 1 and type(rnn) is FusedLSTM and rnn.wgrad is True
        assert list(net.state_dict().keys()) == keys                                     # not in state_dict
        clone = copy.deepcopy(net)
        crnn = [m for m in clone.modules() if isinstance(m, nn.LSTM)][0]
        assert type(crnn) is FusedLSTM and crnn.wgrad is True                            # survives the deep copy
        clone.load_state_dict(lstm_ref.make_network(name, seed=5).state_dict())          # a stock network's file loads unchanged
        assert unfuse_lstm(net) == 1 and type(rnn) is nn.LSTM and 'wgrad' not in rnn.__dict__ and not hasattr(rnn, 'wgrad')
        assert fuse_lstm(net) == 1 and not getattr(rnn, 'wgrad', False)                  # fused again without the mode: off
        assert fuse_lstm(net, wgrad=True) == 0 and rnn.wgrad is True                     # an LSTM that is fused already takes the mode


def test_trainer_switches():
    from multiagent_rl_amd.lstm import FusedLSTM, fuse_trainer, wgrad_trainer
    from multiagent_rl_amd.policy import accelerate_trainer

    class T(object):
        pass
    t = T()
    t.actor, t.critic = lstm_ref.make_network('actor'), lstm_ref.make_network('critic')
    t.target_actor, t.target_critic = copy.deepcopy(t.actor), object()
    with pytest.raises(ValueError, match='no fused LSTM'):
        wgrad_trainer(t)
    with pytest.raises(ValueError, match='no fused LSTM'):
        accelerate_trainer(t, wgrad=True)                                               # refused before anything is patched
    assert not hasattr(t, '_pw_accel') and type(t.actor.bilstm) is nn.LSTM
    assert fuse_trainer(t) == 3 and wgrad_trainer(t, dry=True) == 3
    assert not any(getattr(m, 'wgrad', False) for n in (t.actor, t.critic, t.target_actor) for m in n.modules())
    assert wgrad_trainer(t) == 3
    assert all(m.wgrad for n in (t.actor, t.critic, t.target_actor) for m in n.modules() if type(m) is FusedLSTM)
    assert inspect.signature(accelerate_trainer).parameters['wgrad'].default is False
    examples = os.path.join(ROOT, 'examples')
    sys.path.insert(0, examples)
    try:
        import madr_learner
        import train_batched
    finally:
        sys.path.remove(examples)
    assert inspect.signature(madr_learner.Trainer.__init__).parameters['fused_wgrad'].default is False
    with pytest.raises(ValueError, match='fused_lstm'):
        madr_learner.Trainer(lstm_ref.make_network('actor'), lstm_ref.make_network('critic'), None, device='cpu', fused_wgrad=True)
    learner = madr_learner.Trainer(lstm_ref.make_network('actor'), lstm_ref.make_network('critic'), None, device='cpu', fused_lstm=True,
                                   fused_wgrad=True)
    for net in (learner.actor, learner.critic, learner.target_actor, learner.target_critic):
        assert [m.wgrad for m in net.modules() if type(m) is FusedLSTM] == [True]
    with pytest.raises(SystemExit):
        train_batched.main(['--fused-wgrad'])                                           # needs --fused-lstm


# ---- the C entry points -----------------------------------------------------------------------------------------------------------
P = [4096 + 1024 * k for k in range(6)]    # fake, 4-byte aligned "device pointers": every call below is refused before a launch


def _wgrad(dG=P[0], Y=P[1], b=8, N=6, dirs=1, H=64, fw=P[2], bw=None, scratch=P[4]):
    return _lib.load().pw_lstm_train_wgrad(dG, Y, b, N, dirs, H, fw, bw, scratch, None)


def test_symbols_are_exported_and_declared():
    lib = _lib.load()
    header = open(os.path.join(ROOT, 'include', 'pworld.h')).read()
    assert re.search(r'\bint pw_lstm_train_wgrad\(', header) and re.search(r'\bsize_t pw_lstm_train_wgrad_scratch_bytes\(', header)
    for name in ('pw_lstm_train_wgrad', 'pw_lstm_train_wgrad_scratch_bytes'):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert lib.pw_version() >= 120


@pytest.mark.parametrize('kw,word', [
    (dict(dirs=1, H=32), b'dirs'), (dict(dirs=2, H=64), b'dirs'), (dict(dirs=3, H=32), b'dirs'), (dict(dirs=0), b'dirs'), (dict(H=48), b'H'),
    (dict(N=0), b'N must'), (dict(N=-1), b'N must'), (dict(b=0), b'b must'), (dict(b=-4), b'b must'), (dict(b=1 << 41, N=1), b'b N'),
    (dict(dG=None), b'dG is null'), (dict(Y=None), b'Y is null'), (dict(fw=None), b'both null'),
    (dict(dirs=2, H=32, fw=None, bw=None), b'both null'), (dict(bw=P[3]), b'dw_hh_bw must be null with dirs = 1'),
    (dict(scratch=None), b'scratch is null'),
    (dict(dG=P[0] + 2), b'dG must be 4-byte aligned'), (dict(Y=P[1] + 1), b'Y must be 4-byte aligned'),
    (dict(fw=P[2] + 2), b'dw_hh_fw must be 4-byte aligned'), (dict(dirs=2, H=32, bw=P[3] + 3), b'dw_hh_bw must be 4-byte aligned'),
    (dict(scratch=P[4] + 1), b'scratch must be 4-byte aligned'),
], ids=lambda v: str(v) if isinstance(v, dict) else '')
def test_the_entry_point_refuses_before_anything_is_launched(kw, word):
    assert _wgrad(**kw) == EINVAL
    assert word in _lib.load().pw_last_error(), _lib.load().pw_last_error()


def test_scratch_bytes_follow_from_the_shape():
    """One slot of [4H][H] floats per direction and workgroup; workgroups = tiles of 16 rows shared out evenly over at most 128."""
    f = _lib.load().pw_lstm_train_wgrad_scratch_bytes
    slot = 4 * 256 * 64
    assert f(1, 1, 1, 64) == slot and f(1, 1, 2, 32) == slot // 2
    assert f(1, 16, 1, 64) == slot and f(1, 17, 1, 64) == 2 * slot and f(17, 4, 2, 32) == 5 * slot // 2
    assert f(1024, 6, 1, 64) == 128 * slot                                  # 384 tiles: 3 per workgroup
    assert f(300, 21, 1, 64) == 99 * slot                                   # 394 tiles: 4 per workgroup, 99 workgroups
    assert f(1 << 20, 48, 2, 32) == 128 * slot // 2
    assert f(8, 6, 1, 32) == 0 and f(0, 6, 1, 64) == 0 and f(8, 0, 1, 64) == 0


def test_the_new_unit_carries_exactly_its_own_kernels():
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
    src = open(os.path.join(ROOT, 'multiagent_rl_amd', 'csrc', 'pw_kernels_lstm_wgrad.hpp')).read()
    defined = set(re.findall(r'__global__ void (?:__launch_bounds__\(\w+\) )?(pw_\w+_kernel)\(', src))
    assert defined == {'pw_lstm_train_wgrad_kernel', 'pw_lstm_train_wgrad_reduce_kernel'}
    names = code_object.per_unit_kernels()['pworld_lstm_wgrad']
    assert {re.match(r'(?:void )?(\w+)', n).group(1) for n in names} == defined and len(names) == 3
    assert os.path.join(build_native.HERE, 'csrc', 'pworld_lstm_wgrad.hip') in build_native.SRCS
    assert 'pworld_lstm_wgrad' in build_native.unit_sources.__doc__
    unit = [os.path.basename(f) for f in build_native.unit_sources('pworld_lstm_wgrad')]
    assert 'pw_kernels_lstm_wgrad.hpp' in unit and 'pw_kernels_lstm.hpp' not in unit
