"""CPU: the host side of pw_lstm_train_forward / pw_lstm_train_backward and of multiagent_rl_amd.lstm (no launch happens without a GPU:
every call into the library here is refused before one), the float64 restatement tests/lstm_ref.py against float64 nn.LSTM autograd,
and the Python plumbing (autograd function, FusedLSTM, fuse_lstm) with the two launches replaced by that restatement.

Bounds.  Restatement in float64 against autograd in float64: 1e-12 (the formulas are the same mathematics; what differs is the
summation order of matrix products of at most 64 x 256 terms of size <= ~10: a few 1e-14).  Float32 plumbing against the float64 deep
copy of the network: 4 x max(e_stock, 2^-23 max|ref|) per parameter gradient, e_stock = the unfused float32 network's error in the same
test (the factor is tests/test_gpu_optim.py's for an equally long rounding chain; the second term is one float32 rounding of the
largest entry and keeps an exactly zero stock error, N = 1's weight_hh, from making the ratio meaningless)."""
import copy
import os
import re
import sys

import pytest

from multiagent_rl_amd import _lib
from tests import lstm_ref

torch = pytest.importorskip('torch')
nn = torch.nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


# ---- the restatement --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('b,N,dirs,H', lstm_ref.SHAPES)
def test_restatement_equals_float64_autograd(b, N, dirs, H):
    lstm = lstm_ref.make_lstm(dirs, H, torch.float64)
    x, dY = lstm_ref.make_inputs(b, N, dirs, H, torch.float64)
    ours, ref = lstm_ref.split_grads(lstm, x, dY), lstm_ref.autograd_grads(lstm, x, dY)
    assert set(ref) == set(ours) - {'G', 'dG'} and len(ref) == 2 + 4 * dirs
    for name, r in ref.items():
        err = float((ours[name] - r).abs().max())
        assert err <= 1e-12, (name, err)


# ---- the plumbing, with stand-ins for the two launches ----------------------------------------------------------------------------
@pytest.fixture
def standins(monkeypatch):
    from multiagent_rl_amd import lstm
    monkeypatch.setattr(lstm, 'launch_forward', lstm_ref.launch_forward)
    monkeypatch.setattr(lstm, 'launch_backward', lstm_ref.launch_backward)
    return lstm


@pytest.mark.parametrize('b,N', [(33, 6), (5, 13), (4, 1)])
@pytest.mark.parametrize('name', lstm_ref.NETWORKS)
def test_fused_networks_with_standins_against_float64(standins, name, b, N):
    stock = lstm_ref.make_network(name)
    fused, ref = copy.deepcopy(stock), copy.deepcopy(stock).double()
    assert standins.fuse_lstm(fused) == 1
    inputs = lstm_ref.network_inputs(name, b, N, torch.float32)
    g_ref = lstm_ref.network_grads(ref, tuple(t.double() for t in inputs))
    g_stock, g_fused = lstm_ref.network_grads(stock, inputs), lstm_ref.network_grads(fused, inputs)
    assert set(g_fused) == set(g_ref)
    ratio, worst, e_k, e_s = lstm_ref.worst_ratio(g_fused, g_stock, g_ref)
    print('%s b=%d N=%d: worst %s fused %.3e stock %.3e ratio %.2f' % (name, b, N, worst, e_k, e_s, ratio))
    assert ratio <= 4.0, (worst, e_k, e_s)


@pytest.mark.parametrize('dirs,H', [(1, 64), (2, 32)])
def test_lstm_recurrence_function(standins, dirs, H):
    """The autograd function alone: an expanded zero-stride dY (Y.sum()), N = 1 (zero W_hh gradients), no saving without a gradient."""
    lstm = lstm_ref.make_lstm(dirs, H, torch.float64)
    w_ih, bias, w_fw, w_bw = [None if t is None else t.detach().clone() for t in lstm_ref.projection(lstm)]
    for N in (1, 4):
        x, _ = lstm_ref.make_inputs(3, N, dirs, H, torch.float64)
        G = torch.nn.functional.linear(x, w_ih, bias).view(3, N, dirs, 4 * H).requires_grad_(True)
        ws = [w.requires_grad_(True) for w in (w_fw, w_bw) if w is not None]
        Y = standins.lstm_recurrence(G, *ws)
        grads = torch.autograd.grad(Y.sum(), [G] + ws)
        want = lstm_ref.split_grads(lstm, x, torch.ones_like(Y))
        assert float((Y.detach() - want['Y']).abs().max()) <= 1e-12 and float((grads[0] - want['dG']).abs().max()) <= 1e-12
        for g, key in zip(grads[1:], ('weight_hh_l0', 'weight_hh_l0_reverse')):
            assert float((g - want[key]).abs().max()) <= 1e-12
            assert N > 1 or float(g.abs().max()) == 0.0
    seen = []
    standins.launch_forward = lambda G, a, b, keep: seen.append(keep) or lstm_ref.launch_forward(G, a, b, keep)
    with torch.no_grad():
        standins.lstm_recurrence(G, *ws)
    standins.lstm_recurrence(G.detach(), *[w.detach() for w in ws])
    assert seen == [False, False]


def test_h_n_is_a_slice_of_the_output_and_c_n_carries_no_gradient(standins):
    for dirs, H in ((1, 64), (2, 32)):
        lstm = lstm_ref.make_lstm(dirs, H, torch.float32)
        ref = copy.deepcopy(lstm)
        standins.fuse_lstm(lstm)
        x, _ = lstm_ref.make_inputs(4, 5, dirs, H, torch.float32)
        Y, (h_n, c_n) = lstm(x)
        Yr, (hr, cr) = ref(x)
        assert h_n.shape == hr.shape and c_n.shape == cr.shape
        assert torch.allclose(Y, Yr, atol=1e-6) and torch.allclose(h_n, hr, atol=1e-6) and torch.allclose(c_n, cr, atol=1e-6)
        assert h_n.requires_grad and not c_n.requires_grad
        assert torch.equal(h_n[0], Y[:, -1, :H]) and (dirs == 1 or torch.equal(h_n[1], Y[:, 0, H:]))
        g = torch.autograd.grad(h_n.sum(), lstm.weight_hh_l0)[0]
        gr = torch.autograd.grad(hr.sum(), ref.weight_hh_l0)[0]
        assert torch.allclose(g, gr, atol=1e-5)


# ---- the module surface -----------------------------------------------------------------------------------------------------------
def test_fuse_lstm_is_a_class_swap():
    from multiagent_rl_amd.lstm import FusedLSTM, fuse_lstm, unfuse_lstm
    for name in lstm_ref.NETWORKS:
        net = lstm_ref.make_network(name)
        keys = list(net.state_dict().keys())
        params = [p.data_ptr() for p in net.parameters()]
        rnn = [m for m in net.modules() if isinstance(m, nn.LSTM)]
        assert len(rnn) == 1 and fuse_lstm(net) == 1 and type(rnn[0]) is FusedLSTM
        assert fuse_lstm(net) == 0                       # nothing plain left
        assert list(net.state_dict().keys()) == keys and [p.data_ptr() for p in net.parameters()] == params
        clone = copy.deepcopy(net)
        assert [type(m) for m in clone.modules() if isinstance(m, nn.LSTM)] == [FusedLSTM]
        clone.load_state_dict(lstm_ref.make_network(name, seed=5).state_dict())   # a stock network's file loads unchanged
        assert unfuse_lstm(net) == 1 and type(rnn[0]) is nn.LSTM and unfuse_lstm(net) == 0
        net(*lstm_ref.network_inputs(name, 2, 3, torch.float32))                   # and it is nn.LSTM again: runs on the CPU


def test_fuse_lstm_leaves_what_is_not_served():
    from multiagent_rl_amd.lstm import fuse_lstm
    other = nn.ModuleList([nn.LSTM(64, 48, batch_first=True), nn.LSTM(64, 64, num_layers=2, batch_first=True),
                           nn.LSTM(64, 64), nn.LSTM(64, 32, batch_first=True), nn.LSTM(64, 64, batch_first=True, bidirectional=True),
                           nn.LSTM(64, 64, batch_first=True, bias=False), nn.GRU(64, 64, batch_first=True)])
    assert fuse_lstm(other) == 0 and all(type(m) in (nn.LSTM, nn.GRU) for m in other)
    assert fuse_lstm(object()) == 0


def test_fused_lstm_refusals():
    from multiagent_rl_amd.lstm import FusedLSTM, fuse_lstm
    net = nn.LSTM(64, 64, batch_first=True)
    fuse_lstm(net)
    x = torch.zeros(2, 3, 64)
    with pytest.raises(RuntimeError, match='no CPU fallback'):     # a CPU input raises (the real launch function is in place)
        net(x)
    with pytest.raises(ValueError, match='hx'):
        net(x, (torch.zeros(1, 2, 64), torch.zeros(1, 2, 64)))
    with pytest.raises(RuntimeError, match='float32'):
        net.double()(x.double())
    with pytest.raises(ValueError, match=r'\[b, N'):
        net.float()(x[0])
    for kw, word in ((dict(num_layers=2), 'num_layers'), (dict(proj_size=16), 'proj_size'), (dict(num_layers=2, dropout=0.5), 'num_layers'),
                     (dict(bias=False), 'bias'), (dict(batch_first=False), 'batch_first'), (dict(bidirectional=True), 'hidden units')):
        args = dict(batch_first=True)
        args.update(kw)
        bad = nn.LSTM(64, 64, **args)
        bad.__class__ = FusedLSTM
        with pytest.raises(ValueError, match=word):
            bad(x)
    from multiagent_rl_amd import lstm
    with pytest.raises(ValueError, match='dirs'):
        lstm.lstm_recurrence(torch.zeros(2, 3, 1, 128), torch.zeros(128, 32))
    with pytest.raises(ValueError, match='w_hh_bw'):
        lstm.lstm_recurrence(torch.zeros(2, 3, 2, 128), torch.zeros(128, 32))


def test_trainer_switches_fuse_every_network():
    """accelerate_trainer(lstm=True) takes the target networks too; the example learner's fused_lstm fuses before its deep copies."""
    from multiagent_rl_amd.lstm import FusedLSTM, fuse_trainer

    class T(object):
        pass
    t = T()
    t.actor, t.critic = lstm_ref.make_network('actor'), lstm_ref.make_network('critic')
    t.target_actor, t.target_critic = copy.deepcopy(t.actor), object()    # a wrapped target network is left alone
    assert fuse_trainer(t) == 3
    assert type(t.actor.bilstm) is FusedLSTM and type(t.critic.lstm) is FusedLSTM and type(t.target_actor.bilstm) is FusedLSTM
    import inspect
    from multiagent_rl_amd.policy import accelerate_trainer
    assert inspect.signature(accelerate_trainer).parameters['lstm'].default is False
    sys.path.insert(0, os.path.join(ROOT, 'examples'))
    try:
        import madr_learner
    finally:
        sys.path.pop(0)
    assert inspect.signature(madr_learner.Trainer.__init__).parameters['fused_lstm'].default is False


# ---- the C entry points -----------------------------------------------------------------------------------------------------------
P = [4096 + 1024 * k for k in range(6)]    # fake, 4-byte aligned "device pointers": every call below is refused before a launch


def _fwd(G=P[0], fw=P[1], bw=None, b=8, N=6, dirs=1, H=64, Y=P[3], saved=P[4]):
    return _lib.load().pw_lstm_train_forward(G, fw, bw, b, N, dirs, H, Y, saved, None)


def _bwd(dY=P[0], saved=P[4], fw=P[1], bw=None, b=8, N=6, dirs=1, H=64, dG=P[5]):
    return _lib.load().pw_lstm_train_backward(dY, saved, fw, bw, b, N, dirs, H, dG, None)


def test_symbols_are_exported_and_declared():
    lib = _lib.load()
    for name in ('pw_lstm_train_forward', 'pw_lstm_train_backward'):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
        assert re.search(r'\bint %s\(' % name, open(os.path.join(ROOT, 'include', 'pworld.h')).read())
    assert lib.pw_version() >= 112


@pytest.mark.parametrize('call', [_fwd, _bwd], ids=['forward', 'backward'])
@pytest.mark.parametrize('kw,word', [
    (dict(dirs=1, H=32), b'dirs'), (dict(dirs=2, H=64, bw=P[2]), b'dirs'), (dict(dirs=3, H=32, bw=P[2]), b'dirs'), (dict(dirs=0), b'dirs'),
    (dict(H=48), b'H'), (dict(H=0), b'H'), (dict(H=-64), b'H'),
    (dict(N=0), b'N'), (dict(N=-1), b'N'), (dict(b=0), b'b must'), (dict(b=-4), b'b must'), (dict(b=1 << 40), b'b:'),
    (dict(fw=None), b'w_hh_fw'), (dict(dirs=2, H=32), b'w_hh_bw'), (dict(bw=P[2]), b'w_hh_bw'),
    (dict(fw=P[1] + 2), b'w_hh_fw'), (dict(dirs=2, H=32, bw=P[2] + 1), b'w_hh_bw'),
], ids=lambda v: str(v) if isinstance(v, dict) else '')
def test_both_entry_points_refuse_bad_shared_arguments(call, kw, word):
    assert call(**kw) == EINVAL
    assert word in _lib.load().pw_last_error(), _lib.load().pw_last_error()


def test_entry_points_refuse_bad_buffers():
    lib = _lib.load()
    for shape in (dict(), dict(dirs=2, H=32, bw=P[2])):
        for name in ('G', 'Y'):
            assert _fwd(**dict(shape, **{name: None})) == EINVAL and name.encode() + b' is null' in lib.pw_last_error()
            assert _fwd(**dict(shape, **{name: P[0] + 2})) == EINVAL and name.encode() + b' must be 4-byte aligned' in lib.pw_last_error()
        assert _fwd(**dict(shape, saved=P[4] + 1)) == EINVAL and b'saved must be 4-byte aligned' in lib.pw_last_error()
        for name in ('dY', 'saved', 'dG'):
            assert _bwd(**dict(shape, **{name: None})) == EINVAL and name.encode() + b' is null' in lib.pw_last_error()
            assert _bwd(**dict(shape, **{name: P[0] + 3})) == EINVAL and name.encode() + b' must be 4-byte aligned' in lib.pw_last_error()


# ---- what the compiler made of the new unit ---------------------------------------------------------------------------------------
def test_lstm_unit_carries_exactly_its_own_kernels():
    """Mirrors test_small_units_carry_only_their_own_kernels: the unit includes pw_lstm_math.hpp / pw_common.hpp for their device
    functions and must not pick up a kernel with them; both shapes of both kernels are there."""
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
    src = open(os.path.join(ROOT, 'multiagent_rl_amd', 'csrc', 'pw_kernels_lstm.hpp')).read()
    defined = set(re.findall(r'__global__ void (?:__launch_bounds__\(\w+\) )?(pw_\w+_kernel)\(', src))
    assert defined == {'pw_lstm_train_forward_kernel', 'pw_lstm_train_backward_kernel'}
    names = code_object.per_unit_kernels()['pworld_lstm']
    assert {re.match(r'(?:void )?(\w+)', n).group(1) for n in names} == defined
    assert sorted(re.search(r'<(\d+), (\d+)>', n).groups() for n in names) == [('32', '2'), ('32', '2'), ('64', '1'), ('64', '1')]
    assert os.path.join(build_native.HERE, 'csrc', 'pworld_lstm.hip') in build_native.SRCS


# ---- the LDS layout of the two kernels ----------------------------------------------------------------------------------------------
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc not installed')
def test_lstm_layout_is_aligned_disjoint_and_of_the_expected_size(tmp_path):
    """lstm_train_lds (tests/lds_layout_dump_lstm.hip, compiled for the host alone): both regions 16-byte aligned, disjoint and inside
    ``bytes``; ``bytes`` worked out by hand from the region list -- W_hh of every direction (dirs * 4 H * H floats) + one slot per
    (sequence, direction) of a 256-thread workgroup (256 / H slots of H floats forward, 4 H backward) -- never from the function."""
    import subprocess
    from multiagent_rl_amd import build_native
    exe = str(tmp_path / 'lds_layout_dump_lstm')
    r = subprocess.run([HIPCC, '--offload-host-only', '-std=c++17', '-O1', '-I', os.path.join(build_native.HERE, 'csrc'),
                        '-I', os.path.join(ROOT, 'include'), '-o', exe, os.path.join(ROOT, 'tests', 'lds_layout_dump_lstm.hip')],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    want = {'lstm_train H=64 dirs=1 backward=0': 65536 + 1024, 'lstm_train H=64 dirs=1 backward=1': 65536 + 4096,
            'lstm_train H=32 dirs=2 backward=0': 32768 + 1024, 'lstm_train H=32 dirs=2 backward=1': 32768 + 4096}
    seen = {}
    for line in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines():
        key, nbytes, sig, nums = line.split('\t')
        nums = list(map(int, nums.split()))
        regions = sorted((nums[2 * i], nums[2 * i + 1], int(s.split(':')[1])) for i, s in enumerate(sig.split(',')))
        assert [s.split(':')[0] for s in sig.split(',')] == ['w', 'x']
        end = 0
        for off, size, align in regions:
            assert off % align == 0 and off >= end, (key, regions)
            end = off + size
        assert end <= int(nbytes) <= 160 * 1024, (key, end, nbytes)
        seen[key] = int(nbytes)
    assert seen == want
