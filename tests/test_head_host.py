"""CPU: the host side of pw_head_train_forward / pw_head_train_backward / pw_head_train_scratch_bytes and of multiagent_rl_amd.heads (no
launch happens without a GPU: every call into the library here is refused before one), the float64 restatement tests/head_ref.py
against float64 autograd of the stock expression, and the Python plumbing (autograd function, output_layers, fuse_heads) with the
launches replaced by restatements.

Bound.  Restatement in float64 against autograd in float64: 1e-12 relative to the largest entry (the same mathematics; what differs is
the summation order of dot products of at most 136 terms and of sums over at most 771 rows: a few 1e-14 of the largest entry)."""
import copy
import ctypes
import os
import re
import sys

import pytest

from multiagent_rl_amd import _lib
from tests import attention_ref, dense_ref, head_ref, lstm_ref

torch = pytest.importorskip('torch')
nn = torch.nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
SHAPES = [(1, (1,)), (17, (5,)), (65, (5, 10)), (771, (5, 10, 21)), (63, (16, 16, 104))]


def _f64(inp):
    x, ws, bs = inp
    return x.double(), [w.double() for w in ws], [b.double() for b in bs]


def _dOuts(rows, widths, seed=0):
    g = torch.Generator().manual_seed(rows + seed)
    return [torch.randn(rows, n, dtype=torch.float64, generator=g) for n in widths]


def _rel(x, y):
    return float((x - y).abs().max()) / max(float(y.abs().max()), 1e-300)


# ---- the restatement and its inputs ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('relu', [False, True])
@pytest.mark.parametrize('rows,widths', SHAPES)
def test_restatement_equals_float64_autograd(rows, widths, relu):
    x, ws, bs = _f64(head_ref.make_inputs(rows, widths))
    d = _dOuts(rows, widths)
    for used in (range(len(widths)), [0]):                              # every head has a gradient; only the first
        dOuts = [d[k] if k in used else None for k in range(len(widths))]
        outs_want, want = head_ref.stock_grads(lambda outs: sum((outs[k] * d[k]).sum() for k in used), x, ws, bs, relu)
        outs, got = head_ref.forward(x, ws, bs, relu), head_ref.backward(dOuts, x, ws, relu)
        for o, w in zip(outs, outs_want):
            assert _rel(o, w) <= 1e-12
        assert set(got) == set(want)                                    # a head without a dOut: no dW, no db on either side
        for n in want:
            assert _rel(got[n], want[n]) <= 1e-12, n
        assert float(want['dW0'].abs().max()) > 0


def test_inputs_sit_on_the_masks_edge():
    x = head_ref.make_inputs(65, (5, 10))[0]
    zeros = x[x == 0]
    assert zeros.numel() >= 8 and bool(torch.signbit(zeros).any()) and not bool(torch.signbit(zeros).all())     # +0.0 and -0.0
    assert int((x == head_ref.TINY).sum()) >= 4 and head_ref.TINY > 2.0 ** -126
    assert head_ref.make_inputs(65, (5, 10))[0] is x                    # computed once


# ---- the autograd function, with stand-ins for the launches ------------------------------------------------------------------------
@pytest.fixture
def standins(monkeypatch):
    from multiagent_rl_amd import attention, dense, heads, lstm
    calls = []

    def fwd(x, weights, biases, relu):
        heads._shape(x, weights, biases)
        calls.append(('forward', len(weights), bool(relu)))
        return head_ref.launch_forward(x, weights, biases, relu)

    def bwd(dOuts, x, weights, relu, want_dx):
        calls.append(('backward', tuple(d is not None for d in dOuts), want_dx, all(d is None or d.is_contiguous() for d in dOuts)))
        return head_ref.launch_backward(dOuts, x, weights, relu, want_dx)

    def dense_fwd(x0, x1, w1, b1, w_ih, b_ih, b_hh, keep):
        hid, G = dense_ref.forward(x0, x1, w1, b1, w_ih, b_ih, b_hh)
        return G.to(x0.dtype), (hid.to(x0.dtype) if keep else None)

    def dense_bwd(dG, x0, x1, hid, w1, w_ih, want_dx0, want_dx1):
        r = {k: v.to(x0.dtype) for k, v in dense_ref.backward(dG, x0, x1, hid, w1, w_ih).items()}
        n = len(w_ih)
        return (r['dW1'], r['db1'], [r['dW_ih%d' % d] for d in range(n)], [r['db_gate%d' % d] for d in range(n)],
                r['dx0'].contiguous() if want_dx0 else None, r['dx1'].contiguous() if want_dx1 else None)
    monkeypatch.setattr(heads, 'launch_forward', fwd)
    monkeypatch.setattr(heads, 'launch_backward', bwd)
    monkeypatch.setattr(dense, 'launch_forward', dense_fwd)
    monkeypatch.setattr(dense, 'launch_backward', dense_bwd)
    monkeypatch.setattr(lstm, 'launch_forward', lstm_ref.launch_forward)
    monkeypatch.setattr(lstm, 'launch_backward', lstm_ref.launch_backward)
    monkeypatch.setattr(attention, 'launch_forward', attention_ref.launch_forward)
    monkeypatch.setattr(attention, 'launch_backward', attention_ref.launch_backward)
    heads.calls = calls
    yield heads
    del heads.calls


def _leaves(x, ws, bs, grad=('x', 'params')):
    leaf = lambda t, on: t.detach().clone().requires_grad_(on)  # noqa: E731
    return leaf(x, 'x' in grad), [leaf(w, 'params' in grad) for w in ws], [leaf(b, 'params' in grad) for b in bs]


@pytest.mark.parametrize('relu', [False, True])
def test_head_projection_function(standins, relu):
    rows, widths = 65, (5, 10, 21)
    x, ws, bs = _f64(head_ref.make_inputs(rows, widths))
    d = _dOuts(rows, widths)
    losses = ((lambda o: sum((o[k] * d[k]).sum() for k in range(3)), (True, True, True)),
              (lambda o: sum(t.sum() for t in o), (True, True, True)),             # expanded zero-stride gradients arrive contiguous
              (lambda o: (o[0] * d[0]).sum(), (True, False, False)),               # only the first head is used
              (lambda o: (o[2][:, 3] * d[2][:, 3]).sum() + o[1].sum(), (False, True, True)))
    for loss, used in losses:
        _, want = head_ref.stock_grads(loss, x, ws, bs, relu)
        lx, lw, lb = _leaves(x, ws, bs)
        outs = standins.head_projection(lx, lw, lb, relu=relu)
        assert isinstance(outs, tuple) and [tuple(o.shape) for o in outs] == [(rows, n) for n in widths]
        loss(outs).backward()
        assert standins.calls == [('forward', 3, relu), ('backward', used, True, True)]
        del standins.calls[:]
        assert _rel(lx.grad, want['dx']) <= 1e-12
        for k in range(3):
            if used[k]:
                assert _rel(lw[k].grad, want['dW%d' % k]) <= 1e-12 and _rel(lb[k].grad, want['db%d' % k]) <= 1e-12
            else:                                                       # the parameters of a head without a gradient get None, not zeros
                assert lw[k].grad is None and lb[k].grad is None and 'dW%d' % k not in want


def test_what_is_saved_and_what_is_asked_for(standins):
    x, ws, bs = _f64(head_ref.make_inputs(17, (5, 10)))
    saved = []
    hooks = torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(t) or t, lambda t: t)
    with hooks:
        outs = standins.head_projection(*_leaves(x, ws, bs, ()), relu=True)                  # nothing needs a gradient
    assert not saved and not any(o.requires_grad for o in outs)
    with hooks, torch.no_grad():
        outs = standins.head_projection(*_leaves(x, ws, bs), relu=True)
    assert not saved and all(o.grad_fn is None for o in outs)
    with hooks:
        lx, lw, lb = _leaves(x, ws, bs, ('params',))
        outs = standins.head_projection(lx, lw, lb, relu=True)
    assert len(saved) == 3                                                                   # x and the two weights
    del standins.calls[:]
    sum(o.sum() for o in outs).backward()
    assert standins.calls == [('backward', (True, True), False, True)] and lx.grad is None   # x needs none: no dX is formed
    lx, lw, lb = _leaves(x, ws, bs, ('x',))
    standins.head_projection(lx, lw, lb)[1].sum().backward()
    assert standins.calls[-1] == ('backward', (False, True), True, True) and lw[1].grad is None and lx.grad is not None
    # a single tensor for one head; 3-D x: [b, N, 64] -> [b, N, n]
    x3 = x[:12].reshape(4, 3, 64).clone().requires_grad_()
    (out,) = standins.head_projection(x3, ws[0], bs[0], relu=True)
    assert out.shape == (4, 3, 5)
    want = head_ref.forward(x[:12], ws[:1], bs[:1], True)[0].reshape(4, 3, 5)
    assert _rel(out.detach(), want) <= 1e-12
    out.sum().backward()
    assert x3.grad.shape == x3.shape
    xs = x.t().contiguous().t().requires_grad_()                                             # a strided x is made contiguous
    standins.head_projection(xs, ws, bs)[0].sum().backward()
    assert xs.grad.shape == xs.shape


def test_refusals_and_their_messages():
    from multiagent_rl_amd import heads
    x, ws, bs = head_ref.make_inputs(17, (5, 10))
    z = torch.zeros
    with pytest.raises(RuntimeError, match='no CPU fallback'):          # the real launch function is in place
        heads.head_projection(x, ws, bs)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        heads.launch_backward([z(17, 5), None], x, list(ws), True, True)
    with pytest.raises(ValueError, match='at least one of them a tensor'):
        heads.launch_backward([None, None], x, list(ws), True, True)
    with pytest.raises(ValueError, match='1 to 3 heads'):
        heads.head_projection(x, [ws[0]] * 4, [bs[0]] * 4)
    with pytest.raises(ValueError, match='1 to 3 heads'):
        heads.head_projection(x, ws, bs[:1])
    with pytest.raises(ValueError, match='105 columns wide'):
        heads.head_projection(x, [z(105, 64)], [z(105)])
    with pytest.raises(ValueError, match=r'\[rows, 64\]'):
        heads.head_projection(z(17, 32), ws, bs)
    with pytest.raises(ValueError, match=r'\[b, N, 64\]'):
        heads.head_projection(z(2, 2, 2, 64), ws, bs)
    with pytest.raises(ValueError, match='at least one row'):
        heads.head_projection(z(0, 64), ws, bs)
    with pytest.raises(ValueError, match='head 1'):
        heads.head_projection(x, [ws[0], z(10, 32)], bs)


# ---- the switch on the six networks ------------------------------------------------------------------------------------------------
def _networks():
    from multiagent_rl_amd import critic as cr, policy as pol
    return [('critic', lambda: cr.CriticNetwork(16 + 5), 'attention', 1), ('bicnet', lambda: cr.BiCNetCritic(16 + 5), None, 1),
            ('model critic', lambda: cr.ModelCriticNetwork(16 + 5), 'model', 2), ('actor', lambda: pol.ActorNetwork(16, 5), None, 1),
            ('two heads', lambda: pol.ActorNetwork(16, [5, 3]), None, 2), ('model actor', lambda: pol.ModelActorNetwork(16, 5), None, 2)]


def _inputs(net, b, N):
    g = torch.Generator().manual_seed(b * 10 + N)
    obs = torch.randn(b, N, 16, generator=g)
    if hasattr(net, 'bilstm'):
        return (obs,)
    return obs, torch.nn.functional.one_hot(torch.randint(0, 5, (b, N), generator=g), 5).float()


def _flat(out):
    if isinstance(out, (list, tuple)):
        return [t for o in out for t in _flat(o)]
    return [out]


def _structure(out):
    return [type(out).__name__] + [_structure(o) for o in out] if isinstance(out, (list, tuple)) else tuple(out.shape)


@pytest.mark.parametrize('order', ['front first', 'attention first'])
def test_the_switch_on_all_six_networks(standins, order):
    from multiagent_rl_amd import attention, dense, lstm
    heads = standins
    for name, make, form, n_heads in _networks():
        torch.manual_seed(1)
        net = make()
        with pytest.raises(ValueError, match='%s has not been swapped by dense.fuse_front' % type(net).__name__):
            heads.fuse_heads(net)
        assert lstm.fuse_lstm(net) == 1
        original, keys = type(net), list(net.state_dict())
        stock = {N: net(*_inputs(net, 3, N)) for N in (1, 3)}
        fuse_attn = {'attention': attention.fuse_attention, 'model': attention.fuse_model_attention}.get(form)
        if fuse_attn and order == 'attention first':
            assert fuse_attn(net) == 1
            with pytest.raises(ValueError, match='has not been swapped by dense.fuse_front'):    # the attention swap alone is not enough
                heads.fuse_heads(net)
        assert dense.fuse_front(net) == 1
        if fuse_attn and order == 'front first':
            assert fuse_attn(net) == 1
        swapped = type(net)
        assert heads.fuse_heads(net) == 1 and heads.fuse_heads(net) == 0
        assert type(net) is swapped and net.fused_heads is True and list(net.state_dict()) == keys      # an attribute, not a class
        twin = copy.deepcopy(net)
        assert twin.fused_heads is True and type(twin) is swapped and list(twin.state_dict()) == keys
        for N, want in stock.items():
            del heads.calls[:]
            got = twin(*_inputs(net, 3, N))
            assert heads.calls == [('forward', n_heads, hasattr(net, 'bilstm'))], (name, heads.calls)   # one launch for all heads
            assert _structure(got) == _structure(want), name
            for p, q in zip(_flat(got), _flat(want)):
                assert float((p - q).detach().abs().max()) <= 1e-5, (name, N)
        for p in twin.parameters():
            p.grad = None
        del heads.calls[:]
        _flat(twin(*_inputs(net, 3, 3)))[0].sum().backward()             # only the first output is used
        assert heads.calls[1] == ('backward', (True,) + (False,) * (n_heads - 1), True, True), (name, heads.calls)
        lins = [heads._lin(h) for h in heads._heads_of(twin, 'actor' if hasattr(net, 'bilstm') else attention.critic_form(net)[0])]
        assert lins[0].weight.grad is not None and all(lin.weight.grad is None and lin.bias.grad is None for lin in lins[1:])
        # off again: by unfuse_heads, and by unfuse_front
        assert heads.unfuse_heads(twin) == 1 and heads.unfuse_heads(twin) == 0 and 'fused_heads' not in twin.__dict__
        del heads.calls[:]
        got = twin(*_inputs(net, 3, 3))
        assert not heads.calls and type(twin) is swapped
        assert all(float((p - q).detach().abs().max()) <= 1e-5 for p, q in zip(_flat(got), _flat(stock[3])))
        assert dense.unfuse_front(net) == 1 and 'fused_heads' not in net.__dict__
        if fuse_attn:
            assert isinstance(net, attention._Fused)
            del heads.calls[:]
            net(*_inputs(net, 3, 3))
            assert not heads.calls                                         # the attention swap alone ends with the stock calls
            {'attention': attention.unfuse_attention, 'model': attention.unfuse_model_attention}[form](net)
        assert type(net) is original


def test_a_critic_at_65_agents_with_the_attention_swap_outermost(standins):
    """attention._Fused.forward hands N > 64 to ``self._unfused.forward``, looked up on the instance: with the attention swap over the
    front swap that is the front's forward, which ends in output_layers.  A further class layer for the heads would send it round."""
    from multiagent_rl_amd import attention, critic as cr, dense, lstm
    torch.manual_seed(2)
    net = cr.CriticNetwork(16 + 5)
    lstm.fuse_lstm(net)
    inputs = _inputs(net, 2, 65)
    want = net(*inputs)
    assert dense.fuse_front(net) == 1 and attention.fuse_attention(net) == 1 and standins.fuse_heads(net) == 1
    assert type(net).__mro__[1] is attention.FusedAttention
    got = net(*inputs)
    assert standins.calls == [('forward', 1, False)] and float((got - want).detach().abs().max()) <= 1e-5


def test_containers_other_modules_and_wide_heads(standins):
    from multiagent_rl_amd import critic as cr, dense, lstm, policy as pol
    box = nn.ModuleDict(dict(a=cr.CriticNetwork(21), b=nn.Linear(3, 3), c=nn.LSTM(64, 64, batch_first=True), d=pol.ActorNetwork(16, 5)))
    lstm.fuse_lstm(box)
    assert dense.fuse_front(box) == 2
    assert standins.fuse_heads(box) == 2 and 'fused_heads' not in box['b'].__dict__ and 'fused_heads' not in box['c'].__dict__
    assert standins.fuse_heads(None) == 0 and standins.unfuse_heads(box) == 2 and standins.unfuse_heads(None) == 0
    wide = pol.ActorNetwork(16, 105)
    lstm.fuse_lstm(wide)
    dense.fuse_front(wide)
    with pytest.raises(ValueError, match='105 columns wide'):
        standins.fuse_heads(wide)
    assert 'fused_heads' not in wide.__dict__


def test_trainer_switches_say_what_they_need():
    from multiagent_rl_amd import critic as cr, heads, policy as pol

    class T(object):
        pass
    t = T()
    t.actor, t.critic = pol.ActorNetwork(16, 5), cr.CriticNetwork(21)
    with pytest.raises(ValueError, match='heads=True: ActorNetwork has not been swapped.*front=True'):
        heads.fuse_trainer(t)
    with pytest.raises(ValueError, match='front=True'):                    # refused before anything is patched
        pol.accelerate_trainer(t, heads=True)
    assert not hasattr(t, '_pw_accel')
    sys.path.insert(0, os.path.join(ROOT, 'examples'))
    try:
        import madr_learner
    finally:
        sys.path.pop(0)
    with pytest.raises(ValueError, match='fused_heads needs fused_front'):
        madr_learner.Trainer(t.actor, t.critic, None, fused_heads=True)
    assert heads.HANDED_BACK == ()


# ---- the C entry points: nothing is launched for a bad argument -------------------------------------------------------------------
class _Mem(object):
    """Host memory that is never touched: the refusals come before any launch."""

    def __init__(self):
        self.buf = ctypes.create_string_buffer(64)
        self.base = (ctypes.addressof(self.buf) + 15) & ~15


MEM = _Mem()
P = MEM.base


def _arr(*values):
    arr = (ctypes.c_void_p * 3)()
    for i, v in enumerate(values):
        arr[i] = v
    return arr


def _n(*values):
    return (ctypes.c_int32 * 3)(*values)


def _fwd(X=P, rows=6, relu=1, heads=2, w=None, b=None, n=None, out=None):
    return _lib.load().pw_head_train_forward(X, rows, relu, heads, w or _arr(P, P, P), b or _arr(P, P, P), n or _n(5, 10, 21),
                                             out or _arr(P, P, P), None)


def _bwd(dOut=None, X=P, rows=6, relu=1, heads=2, w=None, n=None, dX=P, dW=None, db=None, scratch=P, scratch_bytes=1 << 30):
    return _lib.load().pw_head_train_backward(dOut or _arr(P, P, P), X, rows, relu, heads, w or _arr(P, P, P), n or _n(5, 10, 21), dX,
                                              dW or _arr(P, P, P), db or _arr(P, P, P), scratch, scratch_bytes, None)


def test_symbols_are_exported_and_declared():
    lib = _lib.load()
    header = open(os.path.join(ROOT, 'include', 'pworld.h')).read()
    for name in ('pw_head_train_forward', 'pw_head_train_backward', 'pw_head_train_scratch_bytes'):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
        assert re.search(r'\b(int|size_t) %s\(' % name, header)
    assert lib.pw_version() >= 121 and 'pworld_head.hip' in header


SHARED = [
    (dict(heads=0), b'heads must'), (dict(heads=4), b'heads must'), (dict(n=_n(0, 10, 21)), b'n: every head'),
    (dict(n=_n(5, 105, 21)), b'n: every head'), (dict(heads=3, n=_n(5, 10, -1)), b'n: every head'), (dict(rows=0), b'rows must'),
    (dict(rows=-5), b'rows must'), (dict(rows=1 << 40), b'rows:'), (dict(X=None), b'null'), (dict(X=P + 2), b'4-byte aligned'),
    (dict(w=_arr(P, None)), b'one tensor per head'), (dict(w=_arr(P + 1, P)), b'4-byte aligned'),
]


@pytest.mark.parametrize('call', [_fwd, _bwd], ids=['forward', 'backward'])
@pytest.mark.parametrize('case', range(len(SHARED)))
def test_both_entry_points_refuse_bad_shared_arguments(call, case):
    kw, word = SHARED[case]
    assert call(**kw) == EINVAL
    assert word in _lib.load().pw_last_error(), _lib.load().pw_last_error()


def test_entry_points_refuse_bad_arguments_of_their_own():
    lib = _lib.load()
    assert _fwd(out=_arr(P, None)) == EINVAL and b'one tensor per head' in lib.pw_last_error()
    assert _fwd(b=_arr(None, P)) == EINVAL and b'one tensor per head' in lib.pw_last_error()
    assert _fwd(out=_arr(P, P + 3)) == EINVAL and b'4-byte aligned' in lib.pw_last_error()
    assert _bwd(scratch=None) == EINVAL and b'null' in lib.pw_last_error()
    assert _bwd(dOut=_arr(None, None), dW=_arr(), db=_arr()) == EINVAL and b'every head' in lib.pw_last_error()                      # every dOut NULL
    assert _bwd(dOut=_arr(P, None)) == EINVAL and b'dW and db of a head whose dOut is NULL' in lib.pw_last_error()   # a dW for a NULL dOut
    assert _bwd(dOut=_arr(P, None), dW=_arr(P, None)) == EINVAL and b'dW and db of a head whose dOut is NULL' in lib.pw_last_error()
    assert _bwd(dW=_arr(P, None)) == EINVAL and b'one tensor per head that has a dOut' in lib.pw_last_error()
    assert _bwd(db=_arr(None, P)) == EINVAL and b'one tensor per head that has a dOut' in lib.pw_last_error()
    assert _bwd(dX=P + 4) == EINVAL and b'16-byte aligned' in lib.pw_last_error()
    assert _bwd(dOut=_arr(P + 2, P)) == EINVAL and b'4-byte aligned' in lib.pw_last_error()
    assert _bwd(scratch_bytes=16) == EINVAL and b'scratch_bytes' in lib.pw_last_error()


def test_scratch_size_and_split_follow_from_the_shape_alone():
    q = _lib.load().pw_head_train_scratch_bytes
    per = lambda *n: 4 * sum(64 * k + 2 * k for k in n)  # noqa: E731  (dW, and db as a pair of numbers per column)
    assert q(1, 1, _n(5)) == per(5) and q(16, 2, _n(5, 10)) == per(5, 10) and q(17, 2, _n(5, 10)) == 2 * per(5, 10)
    assert q(128 * 16, 3, _n(16, 16, 104)) == 128 * per(16, 16, 104)
    assert q(128 * 16 + 1, 3, _n(16, 16, 104)) == 65 * per(16, 16, 104)      # two tiles per workgroup from here, and the last owns one
    assert q(6144, 1, _n(5)) == 128 * per(5) and q(1024, 1, _n(1)) == 64 * per(1)
    assert q(0, 1, _n(5)) == 0 and q(6, 4, _n(5, 5, 5)) == 0 and q(6, 1, _n(105)) == 0 and q(6, 0, _n(5)) == 0 and q(6, 1, None) == 0


# ---- what the compiler made of the new unit ---------------------------------------------------------------------------------------
def test_head_unit_carries_exactly_its_own_kernels():
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
    src = open(os.path.join(ROOT, 'multiagent_rl_amd', 'csrc', 'pw_kernels_head.hpp')).read()
    defined = set(re.findall(r'__global__ void (?:__launch_bounds__\(\w+\) )?(pw_\w+_kernel)\(', src))
    assert defined == {'pw_head_train_forward_kernel', 'pw_head_train_backward_kernel', 'pw_head_train_reduce_kernel'}
    names = code_object.per_unit_kernels()['pworld_head']
    assert len(names) == 3 and {re.match(r'(?:void )?(\w+)', n).group(1) for n in names} == defined
    assert os.path.join(build_native.HERE, 'csrc', 'pworld_head.hip') in build_native.SRCS
    assert 'pworld_head' in build_native.unit_sources.__doc__
    unit = [os.path.basename(f) for f in build_native.unit_sources('pworld_head')]
    assert 'pw_kernels_head.hpp' in unit and 'pw_kernels_front.hpp' not in unit
