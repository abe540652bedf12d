"""CPU: the host side of pw_adam_step / pw_soft_update and of multiagent_rl_amd.optim (no launch happens without a GPU: every call here
is refused before one), and the float64 restatement tests/optim_ref.py against float64 torch.optim.Adam + clip_grad_norm_."""
import copy
import ctypes as C

import numpy as np
import pytest

from multiagent_rl_amd import _lib
from tests import optim_ref

torch = pytest.importorskip('torch')

EINVAL = -1


def _table(n, numel=16, target=True):
    rows = [(4096 + 64 * k, 8192 + 64 * k, 12288 + 64 * k, 16384 + 64 * k, (20480 + 64 * k) if target else None, numel)
            for k in range(n)]       # fake, 4-byte aligned "device pointers": every call below is refused before a launch
    return (_lib.PwOptTensor * n)(*rows)


def _adam(table, count, step=1, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.0, max_norm=0.5, tau=0.01):
    return _lib.load().pw_adam_step(table, count, step, lr, b1, b2, eps, wd, max_norm, tau, None, None)


def test_symbols_are_exported_and_declared():
    lib = _lib.load()
    for name in ('pw_adam_step', 'pw_soft_update'):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert C.sizeof(_lib.PwOptTensor) == 48 and _lib.PW_OPT_MAX_TENSORS == 32
    assert lib.pw_version() >= 108


@pytest.mark.parametrize('kw,word', [
    (dict(count=0), b'count'), (dict(count=33), b'count'),
    (dict(step=0), b'step'), (dict(step=-3), b'step'),
    (dict(lr=-1e-3), b'lr'), (dict(lr=float('nan')), b'lr'), (dict(lr=float('inf')), b'lr'),
    (dict(b1=1.0), b'beta'), (dict(b1=-0.1), b'beta'), (dict(b2=1.0), b'beta'), (dict(b2=float('nan')), b'beta'),
    (dict(eps=-1e-8), b'eps'), (dict(eps=float('nan')), b'eps'),
    (dict(wd=-0.1), b'weight_decay'),
    (dict(tau=1.5), b'tau'), (dict(tau=-0.1), b'tau'), (dict(tau=float('nan')), b'tau'),
    (dict(max_norm=float('nan')), b'max_norm'),
], ids=lambda v: str(v) if isinstance(v, dict) else '')
def test_adam_step_refuses_bad_scalars(kw, word):
    lib = _lib.load()
    kw = dict(kw)
    count = kw.pop('count', 4)
    assert _adam(_table(33), count, **kw) == EINVAL
    assert word in lib.pw_last_error(), lib.pw_last_error()


def test_adam_step_refuses_bad_tables():
    lib = _lib.load()
    assert lib.pw_adam_step(None, 1, 1, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0.5, 0.01, None, None) == EINVAL and b'null' in lib.pw_last_error()
    for field in ('param', 'grad', 'exp_avg', 'exp_avg_sq'):
        t = _table(3)
        setattr(t[1], field, None)
        assert _adam(t, 3) == EINVAL and b'null' in lib.pw_last_error(), field
    t = _table(3)
    t[2].numel = 0
    assert _adam(t, 3) == EINVAL and b'numel' in lib.pw_last_error()
    t = _table(3)
    t[0].grad = 8193
    assert _adam(t, 3) == EINVAL and b'aligned' in lib.pw_last_error()
    # 2^20 elements pass the size check, one more does not (16 tensors of 65536 + 1 element in the last)
    t = _table(16, numel=65536)
    t[15].numel = 65537
    assert _adam(t, 16) == EINVAL and b'2^20' in lib.pw_last_error()
    # tau is not looked at when no tensor has a target
    t = _table(2, target=False)
    t[1].numel = -5
    assert _adam(t, 2, tau=7.0) == EINVAL and b'numel' in lib.pw_last_error()


def test_soft_update_refusals():
    lib = _lib.load()
    n = 33
    tp = (C.c_void_p * n)(*[4096 + 64 * k for k in range(n)])
    sp = (C.c_void_p * n)(*[65536 + 64 * k for k in range(n)])
    ne = (C.c_int64 * n)(*[16] * n)
    for count in (0, 33, -1):
        assert lib.pw_soft_update(tp, sp, ne, count, 0.01, None) == EINVAL and b'count' in lib.pw_last_error()
    for tau in (-0.01, 1.01, float('nan')):
        assert lib.pw_soft_update(tp, sp, ne, 4, tau, None) == EINVAL and b'tau' in lib.pw_last_error()
    assert lib.pw_soft_update(None, sp, ne, 4, 0.01, None) == EINVAL and b'null' in lib.pw_last_error()
    assert lib.pw_soft_update(tp, None, ne, 4, 0.01, None) == EINVAL
    assert lib.pw_soft_update(tp, sp, None, 4, 0.01, None) == EINVAL
    sp[2] = None
    assert lib.pw_soft_update(tp, sp, ne, 4, 0.01, None) == EINVAL and b'null' in lib.pw_last_error()
    sp[2] = 65536
    ne[3] = 0
    assert lib.pw_soft_update(tp, sp, ne, 4, 0.01, None) == EINVAL and b'numel' in lib.pw_last_error()
    ne[3] = (1 << 20) - 47
    assert lib.pw_soft_update(tp, sp, ne, 4, 0.01, None) == EINVAL and b'2^20' in lib.pw_last_error()
    tp[0] = 4097
    ne[3] = 16
    assert lib.pw_soft_update(tp, sp, ne, 4, 0.01, None) == EINVAL and b'aligned' in lib.pw_last_error()


def _net():
    torch.manual_seed(3)
    return torch.nn.Sequential(torch.nn.Linear(7, 5), torch.nn.Linear(5, 3))


def test_state_dict_round_trip_with_torch_adam():
    from multiagent_rl_amd.optim import FusedAdam
    net = _net()
    adam = torch.optim.Adam(net.parameters(), lr=3e-3, betas=(0.8, 0.99), eps=1e-7, weight_decay=1e-4, foreach=False)
    for _ in range(3):
        adam.zero_grad()
        net(torch.randn(11, 7)).square().sum().backward()
        adam.step()
    fused = FusedAdam(net.parameters(), lr=1.0)
    assert set(fused.defaults) == set(adam.defaults)
    assert set(fused.param_groups[0]) == set(adam.param_groups[0])
    fused.load_state_dict(adam.state_dict())
    g = fused.param_groups[0]
    assert (g['lr'], g['betas'], g['eps'], g['weight_decay']) == (3e-3, (0.8, 0.99), 1e-7, 1e-4)
    for p in net.parameters():
        assert sorted(fused.state[p]) == ['exp_avg', 'exp_avg_sq', 'step'] and float(fused.state[p]['step']) == 3.0
        assert torch.equal(fused.state[p]['exp_avg'], adam.state[p]['exp_avg'])
    # and back: a fresh torch Adam takes the fused optimiser's state_dict and goes on stepping
    back = torch.optim.Adam(net.parameters(), foreach=False)
    back.load_state_dict(copy.deepcopy(fused.state_dict()))      # (load_state_dict shares the state tensors it is given)
    assert back.param_groups[0]['lr'] == 3e-3 and back.param_groups[0]['betas'] == (0.8, 0.99)
    twin = _net()
    twin.load_state_dict(net.state_dict())
    twin_adam = torch.optim.Adam(twin.parameters(), foreach=False)
    twin_adam.load_state_dict(copy.deepcopy(adam.state_dict()))
    x = torch.randn(11, 7)
    for n_, o_ in ((net, back), (twin, twin_adam)):
        o_.zero_grad()
        n_(x).square().sum().backward()
        o_.step()
    assert all(torch.equal(a, b) for a, b in zip(net.parameters(), twin.parameters()))
    # from_adam: the same in one call
    again = FusedAdam.from_adam(adam)
    assert again.param_groups[0]['eps'] == 1e-7 and float(again.state[next(net.parameters())]['step']) == 3.0


def test_what_the_python_surface_refuses():
    from multiagent_rl_amd import optim
    net = _net()
    net(torch.randn(4, 7)).sum().backward()
    opt = optim.FusedAdam(net.parameters(), lr=1e-3)
    before = [p.detach().clone() for p in net.parameters()]
    with pytest.raises(RuntimeError, match='GPU'):
        opt.step()                                                     # CPU parameters: no fallback
    assert all(torch.equal(a, b) for a, b in zip(before, net.parameters()))
    with pytest.raises(ValueError):
        optim.FusedAdam(net.parameters(), lr=1e-3, amsgrad=True)
    with pytest.raises(ValueError):
        optim.FusedAdam(net.parameters(), lr=1e-3, maximize=True)
    with pytest.raises(ValueError):
        optim.FusedAdam(net.parameters(), lr=1e-3, targets=list(_net().parameters()))          # targets without tau
    with pytest.raises(ValueError):
        optim.FusedAdam(net.parameters(), lr=1e-3, targets=list(_net().parameters())[:3], tau=0.01)
    with pytest.raises(ValueError):
        optim.FusedAdam(net.parameters(), lr=-1.0)
    with pytest.raises(ValueError):
        optim.FusedAdam(net.parameters(), lr=1e-3, max_norm=0.0)
    with pytest.raises(RuntimeError, match='GPU'):
        optim.soft_update(_net(), net, 0.01)
    # AdamW's decay (decoupled_weight_decay, where the installed torch's Adam has the key) is not the kernel's L2 form
    adamw = torch.optim.AdamW(net.parameters(), lr=1e-3)
    if 'decoupled_weight_decay' in adamw.defaults:
        with pytest.raises(ValueError, match='decoupled_weight_decay'):
            optim.FusedAdam.from_adam(adamw)
        with pytest.raises(ValueError, match='decoupled_weight_decay'):
            optim.FusedAdam(net.parameters(), lr=1e-3).load_state_dict(adamw.state_dict())
        opt.param_groups[0]['decoupled_weight_decay'] = True
        with pytest.raises(ValueError, match='decoupled_weight_decay'):
            opt.step()

        class _Holder(object):
            actor_optimizer = critic_optimizer = adamw
        with pytest.raises(ValueError, match='decoupled_weight_decay'):
            optim.fuse_optimizers(_Holder())


@pytest.mark.parametrize('scale,wd', [(1e-3, 0.0), (1.0, 0.0), (30.0, 0.0), (1.0, 1e-2)], ids=lambda v: str(v))
def test_float64_restatement_agrees_with_float64_torch(scale, wd):
    """25 steps of clip_grad_norm_(0.5) + torch.optim.Adam(foreach=False) in float64 against tests/optim_ref.py: 1e-12."""
    rng = np.random.RandomState(5)
    shapes = [(1,), (3,), (64, 21), (256, 64), (65,), (5, 64)]
    start = [rng.randn(*s) * 0.1 for s in shapes]
    lr, betas, eps, max_norm = 1e-2, (0.9, 0.999), 1e-8, 0.5
    params = [torch.tensor(x, dtype=torch.float64, requires_grad=True) for x in start]
    adam = torch.optim.Adam(params, lr=lr, betas=betas, eps=eps, weight_decay=wd, foreach=False)
    ref = optim_ref.AdamF64(start, lr=lr, betas=betas, eps=eps, weight_decay=wd, max_norm=max_norm)
    for it in range(25):
        grads = [rng.randn(*s) * scale for s in shapes]
        skip = 2 if it % 5 == 4 else None                              # a parameter without gradient now and then
        for i, (p, g) in enumerate(zip(params, grads)):
            p.grad = None if i == skip else torch.tensor(g)
        live = [p for p in params if p.grad is not None]
        norm = torch.nn.utils.clip_grad_norm_(live, max_norm, foreach=False)
        adam.step()
        ref.step([None if i == skip else g for i, g in enumerate(grads)])
        assert abs(float(norm) - ref.total_norm) <= 1e-12 * ref.total_norm
    for p, q, shape in zip(params, ref.p, shapes):
        assert float(np.abs(p.detach().numpy() - q).max()) <= 1e-12, shape
    for p, m, v in zip(params, ref.m, ref.v):
        assert float(np.abs(adam.state[p]['exp_avg'].numpy() - m).max()) <= 1e-12
        assert float(np.abs(adam.state[p]['exp_avg_sq'].numpy() - v).max()) <= 1e-12


def test_float32_soft_update_restatement_is_torchs_expression_bit_for_bit():
    rng = np.random.RandomState(9)
    t, s = rng.randn(4099).astype(np.float32), rng.randn(4099).astype(np.float32)
    for tau in (1e-2, 0.5, 0.3, 1e-3):
        want = (torch.from_numpy(t) * (1.0 - tau) + torch.from_numpy(s) * tau).numpy()
        assert np.array_equal(optim_ref.soft_update_f32(t, s, tau).view(np.uint32), want.view(np.uint32)), tau
    t[5] = np.inf
    assert np.array_equal(optim_ref.soft_update_f32(t, s, 1.0).view(np.uint32), s.view(np.uint32))
