"""GPU: pw_front_train_forward / pw_front_train_backward and their Python surface (multiagent_rl_amd.dense: front_projection, fuse_front,
the example learner's fused_front switch).

Reference: tests/dense_ref.py, the float64 restatement (forward from the inputs; backward from the DEVICE's own hid, ``hid > 0`` the mask).
Bound, the project's own (tests/lstm_ref.worst_ratio <= 4): the error against float64 is at most 4 x max(the stock float32 expression's
error in the same run, one float32 rounding of the reference's largest entry).  Inputs keep every ReLU pre-activation 1e-5 away from zero
(dense_ref.make_inputs), so float32 and float64 agree on the mask.
"""
import copy
import functools

import pytest
import torch

from tests import dense_ref, lstm_ref

pytestmark = pytest.mark.gpu

ROWS = (1, 6, 63, 65, 771, 6144)
WIDTHS = ((1, 0), (16, 5), (21, 15), (103, 16), (104, 16))
EINVAL = -1

# the three gradient patterns: (name, the loss autograd sees, the dG it amounts to)
PATTERNS = (
    ('random dG', lambda G, d: (G * d).sum(), lambda d: d),
    ('G.sum() (expanded dG)', lambda G, d: G.sum(), lambda d: torch.ones_like(d)),
    ('only column 5', lambda G, d: (G[:, 5] * d[:, 5]).sum(), lambda d: torch.zeros_like(d).index_copy_(1, torch.tensor([5]), d[:, 5:6])),
)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _check(tag, kernel, stock, ref):
    for n in ref:
        assert n in kernel and bool(torch.isfinite(kernel[n]).all()), (tag, n)
    ratio, worst, e_k, e_s = lstm_ref.worst_ratio(kernel, stock, ref)
    print('%-60s worst %-10s kernel %.3e  stock %.3e  ratio %.2f' % (tag, worst, e_k, e_s, ratio))
    assert ratio <= 4.0, (tag, worst, e_k, e_s, ratio)


@functools.lru_cache(maxsize=None)
def _case(rows, d0, d1, dirs):
    """-> (inputs on the device, the float64 forward (hid, G) on the CPU, dG float32 on the CPU); computed once and left unchanged."""
    inp = dense_ref.make_inputs(rows, d0, d1, dirs)
    names = ('x0', 'x1', 'w1', 'b1', 'w_ih', 'b_ih', 'b_hh')
    cpu = {k: inp[k] for k in names}
    up = lambda t: None if t is None else t.cuda()  # noqa: E731
    dev = {k: ([up(t) for t in v] if isinstance(v, tuple) else up(v)) for k, v in cpu.items()}
    dG = torch.randn(rows, 256, generator=torch.Generator().manual_seed(rows + d0))
    return dev, dense_ref.forward(**cpu), dG


def _leaves(dev):
    leaf = lambda t: None if t is None else t.detach().clone().requires_grad_()  # noqa: E731
    return {k: ([leaf(t) for t in v] if isinstance(v, list) else leaf(v)) for k, v in dev.items()}


def _named_grads(v):
    out = dict(dW1=v['w1'].grad, db1=v['b1'].grad, dx0=v['x0'].grad)
    if v['x1'] is not None:
        out['dx1'] = v['x1'].grad
    for d in range(len(v['w_ih'])):
        out['dW_ih%d' % d], out['db_gate%d' % d] = v['w_ih'][d].grad, v['b_ih'][d].grad
    return out


# ---- 1. accuracy ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dirs', [1, 2], ids=['1x64', '2x32'])
@pytest.mark.parametrize('d0,d1', WIDTHS)
def test_front_projection_against_float64(d0, d1, dirs):
    from multiagent_rl_amd import dense
    for rows in ROWS:
        dev, (_, G_ref), dG = _case(rows, d0, d1, dirs)
        hid = dense.launch_forward(dev['x0'], dev['x1'], dev['w1'], dev['b1'], dev['w_ih'], dev['b_ih'], dev['b_hh'], True)[1]
        cpu64 = lambda t: None if t is None else t.detach().double().cpu()  # noqa: E731
        for name, loss, as_dG in PATTERNS:
            d = dG.cuda()
            v = _leaves(dev)
            G = dense.front_projection(**v)
            loss(G, d).backward()
            kernel = dict(_named_grads(v), G=G.detach())
            for k in range(dirs):                                     # b_hh receives what b_ih receives
                assert torch.equal(_bits(v['b_hh'][k].grad), _bits(v['b_ih'][k].grad))
            G_stock, stock = dense_ref.stock_grads(lambda g: loss(g, d), **dev)
            ref = dense_ref.backward(as_dG(dG), cpu64(dev['x0']), cpu64(dev['x1']), cpu64(hid), cpu64(dev['w1']), [cpu64(t) for t in dev['w_ih']])
            _check('rows %d d0 %d d1 %d dirs %d %s' % (rows, d0, d1, dirs, name), kernel, dict(stock, G=G_stock), dict(ref, G=G_ref))
            assert float(kernel['dW1'].abs().max()) > 0


# ---- 2. determinism ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dirs', [1, 2], ids=['1x64', '2x32'])
@pytest.mark.parametrize('rows', [6144, 771])
def test_the_same_inputs_give_the_same_bits(rows, dirs):
    from multiagent_rl_amd import dense
    dev, _, dG = _case(rows, 16, 5, dirs)
    d = dG.cuda()

    def run(a, g):
        G, hid = dense.launch_forward(a['x0'], a['x1'], a['w1'], a['b1'], a['w_ih'], a['b_ih'], a['b_hh'], True)
        dW1, db1, dW_ih, db_gate, dx0, dx1 = dense.launch_backward(g, a['x0'], a['x1'], hid, a['w1'], a['w_ih'], True, True)
        return [G, hid, dW1, db1, dx0, dx1] + dW_ih + db_gate
    first, second = run(dev, d), run(dev, d)
    other, _, other_dG = _case(65, 21, 15, dirs)                       # an unrelated launch of another shape in between
    run(other, other_dG.cuda())
    third = run(dev, d)
    for i, (a, b, c) in enumerate(zip(first, second, third)):
        assert torch.equal(_bits(a), _bits(b)) and torch.equal(_bits(a), _bits(c)), i


# ---- 3. kernel count -----------------------------------------------------------------------------------------------------------------
def _device_kernels(fn):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        out = fn()
        torch.cuda.synchronize()
    return out, [e.name for e in prof.events() if str(getattr(e, 'device_type', '')).endswith('CUDA')]


def test_one_kernel_forward_and_two_backward():
    from multiagent_rl_amd import dense
    dev, _, dG = _case(6144, 16, 5, 1)
    v, d = _leaves(dev), dG.cuda()
    leaves = [v['x0'], v['x1'], v['w1'], v['b1']] + v['w_ih'] + v['b_ih'] + v['b_hh']
    torch.autograd.grad(dense.front_projection(**v), leaves, d)          # warm: the library is loaded, the allocator has its blocks
    torch.cuda.synchronize()
    G, fwd = _device_kernels(lambda: dense.front_projection(**v))
    _, bwd = _device_kernels(lambda: torch.autograd.grad(G, leaves, d))
    print('forward: %r\nbackward: %r' % (fwd, bwd))
    assert len(fwd) == 1 and 'pw_front_train_forward_kernel' in fwd[0]
    assert 1 <= len(bwd) <= 2 and 'pw_front_train_backward_kernel' in bwd[0] and all('pw_front_train' in k for k in bwd)


# ---- 4. module level -----------------------------------------------------------------------------------------------------------------
def _flat(out):
    if isinstance(out, (list, tuple)):
        return [t for o in out for t in _flat(o)]
    return [out]


NETWORKS = {
    'CriticNetwork': lambda pol, cr: cr.CriticNetwork(16 + 5),
    'BiCNetCritic': lambda pol, cr: cr.BiCNetCritic(16 + 5),
    'ModelCriticNetwork': lambda pol, cr: cr.ModelCriticNetwork(16 + 5),
    'ActorNetwork': lambda pol, cr: pol.ActorNetwork(16, 5),
    'ActorNetwork two heads': lambda pol, cr: pol.ActorNetwork(16, [5, 3]),
    'ModelActorNetwork': lambda pol, cr: pol.ModelActorNetwork(16, 5),
}


def _outputs_and_grads(net, inputs, weights):
    for p in net.parameters():
        p.grad = None
    outs = _flat(net(*inputs))
    sum((o * w.to(o)).sum() for o, w in zip(outs, weights)).backward()
    res = {'out%d' % i: o.detach() for i, o in enumerate(outs)}
    res.update({n: p.grad.detach().clone() for n, p in net.named_parameters()})
    return res


@pytest.mark.parametrize('name', list(NETWORKS))
def test_swapped_networks_against_float64(name):
    from multiagent_rl_amd import critic as cr, dense, lstm, policy as pol
    torch.manual_seed(11)
    plain = NETWORKS[name](pol, cr)
    ref_net = copy.deepcopy(plain).double()
    stock_net = copy.deepcopy(plain).cuda()
    assert lstm.fuse_lstm(stock_net) == 1
    fused_net = copy.deepcopy(stock_net)
    assert dense.fuse_front(fused_net) == 1 and isinstance(fused_net, type(plain))
    b = 257
    for N in (1, 3, 6):
        g = torch.Generator().manual_seed(N)
        obs = torch.randn(b, N, 16, generator=g)
        inputs = (obs,)
        if not hasattr(plain, 'bilstm'):
            inputs = (obs, torch.nn.functional.one_hot(torch.randint(0, 5, (b, N), generator=g), 5).float())
        outs = _flat(ref_net(*[t.double() for t in inputs]))
        weights = [torch.randn(o.shape, generator=g) for o in outs]
        ref = _outputs_and_grads(ref_net, [t.double() for t in inputs], weights)
        dev_in = [t.cuda() for t in inputs]
        _check('%s b %d N %d' % (name, b, N), _outputs_and_grads(fused_net, dev_in, weights), _outputs_and_grads(stock_net, dev_in, weights), ref)
    unswapped = copy.deepcopy(stock_net)
    with torch.no_grad():
        for p in unswapped.parameters():
            p.zero_()
    unswapped.load_state_dict(fused_net.state_dict())                      # strict: the keys are the unswapped network's
    assert list(unswapped.state_dict()) == list(fused_net.state_dict())
    assert all(torch.equal(p, q) for p, q in zip(unswapped.state_dict().values(), fused_net.state_dict().values()))
    fused_net.load_state_dict(unswapped.state_dict())
    assert dense.unfuse_front(fused_net) == 1 and type(fused_net) is type(stock_net)


# ---- 5. the capability: graphed and eager updates with the fused front, bit for bit --------------------------------------------------
def _learner(ug, variant, nets, graph, front=True):
    import madr_learner
    from multiagent_rl_amd.policy import accelerate_trainer
    cls_name, _, _, ring_kw, N, D = ug.VARIANTS[variant]
    actor, critic = copy.deepcopy(nets)
    t = getattr(madr_learner, cls_name)(actor, critic, ug._filled_memory(ring_kw, N, D),
                                        action_type='MultiDiscrete' if 'act_heads' in ring_kw else 'Discrete', batch_size=ug.BATCH,
                                        fused_optimizer=True, fused_lstm=True, fused_attention=True, graph_update=graph,
                                        fused_sampling=True, sampling_seed=5, fused_front=front)
    if not graph:
        accelerate_trainer(t, targets=True)
    return t


@pytest.mark.parametrize('variant', ['attention', 'two_head', 'bicnet', 'model'])
def test_graphed_updates_with_the_fused_front_equal_eager_updates_bit_for_bit(variant):
    """Learners A and B eager, C graphed, all with fused_front: A == B == C in every parameter, target, Adam moment and loss after each
    of 8 updates and after a learning-rate change (a re-capture).  Learner D, without the switch, starts from the same weights: after
    the first update both losses agree with A's to 1e-3 relative (one update from identical weights: only the summation order differs),
    and after 8 updates some parameter differs."""
    import tests.test_gpu_update_graph as ug                              # the harness: VARIANTS, _filled_memory, _everything, _same
    from multiagent_rl_amd import critic as cr, dense, policy as pol
    from multiagent_rl_amd.graph import GraphedUpdate
    torch.manual_seed(3)
    nets = (ug.VARIANTS[variant][1](pol, cr), ug.VARIANTS[variant][2](pol, cr))
    a, b, c = (_learner(ug, variant, nets, graph) for graph in (False, False, True))
    d = _learner(ug, variant, nets, False, front=False)
    assert isinstance(c.optimize, GraphedUpdate)
    for t in (a, b, c):
        assert isinstance(t.actor, dense.FusedFront) and isinstance(t.critic, dense.FusedFront)
    assert not isinstance(d.actor, dense.FusedFront) and not isinstance(d.critic, dense.FusedFront)

    def step(t, k):
        torch.manual_seed(100 + k)
        return tuple(float(x) for x in t.optimize())
    for it in range(8):
        la, lb, lc, ld = step(a, 0), step(b, 1), step(c, 2), step(d, 3)
        sa, sb, sc = ug._everything(a), ug._everything(b), ug._everything(c)
        assert len(sa) == len(sc) > 20
        bad_b = [i for i, (x, y) in enumerate(zip(sa, sb)) if not ug._same(x, y)]
        bad_c = [i for i, (x, y) in enumerate(zip(sa, sc)) if not ug._same(x, y)]
        print('%s update %d: losses A %r B %r C %r D %r; tensors differing A/B %r A/C %r' % (variant, it + 1, la, lb, lc, ld, bad_b[:5], bad_c[:5]))
        assert la == lb and not bad_b, (variant, it)
        assert la == lc and not bad_c, (variant, it)
        if it == 0:
            for x, y in zip(la, ld):
                assert abs(x - y) <= 1e-3 * abs(y), (la, ld)
    assert any(not ug._same(x, y) for x, y in zip(ug._everything(a), ug._everything(d)))
    g = c.optimize
    assert (g.eager_calls, g.captures, g.replays) == (3, 1, 5)
    for t in (a, c):                                                       # a changed learning rate: captured again, still the eager learner's bits
        for opt in (t.actor_optimizer, t.critic_optimizer):
            opt.param_groups[0]['lr'] = 1e-3
    la, lc = step(a, 0), step(c, 2)
    assert g.captures == 2 and la == lc and all(ug._same(x, y) for x, y in zip(ug._everything(a), ug._everything(c)))


def test_accelerate_trainer_front_switch():
    """front=True needs fused LSTMs (its own lstm=True counts) and reaches the target networks that are still modules."""
    import madr_learner
    import tests.test_gpu_update_graph as ug
    from multiagent_rl_amd import critic as cr, dense, policy as pol
    _, mk_actor, mk_critic, ring_kw, N, D = ug.VARIANTS['attention']
    make = lambda **kw: madr_learner.Trainer(mk_actor(pol, cr), mk_critic(pol, cr), ug._filled_memory(ring_kw, N, D), batch_size=ug.BATCH, **kw)  # noqa: E731
    with pytest.raises(ValueError, match='plain nn.LSTM'):
        pol.accelerate_trainer(make(), front=True)
    with pytest.raises(ValueError, match='plain nn.LSTM'):
        make(fused_front=True)
    t = make()
    fx = pol.accelerate_trainer(t, lstm=True, attention=True, front=True)
    assert fx.fused_fronts == 4 and all(isinstance(n, dense.FusedFront) for n in (t.actor, t.critic, t.target_actor, t.target_critic))
    la, lc = t.optimize()
    assert la == la and lc == lc
    t = make(fused_lstm=True)
    fx = pol.accelerate_trainer(t, targets=True, front=True)                 # the targets are wrappers on the no-gradient kernels: left alone
    assert fx.fused_fronts == 2 and isinstance(t.critic, dense.FusedFront)


# ---- 6. refusals on the device -------------------------------------------------------------------------------------------------------
def test_refusals_on_the_device():
    from multiagent_rl_amd import _lib, dense
    dev, _, _ = _case(6, 16, 5, 1)
    args = lambda **kw: {**dev, **kw}  # noqa: E731
    z = lambda *s: torch.zeros(*s, device='cuda')  # noqa: E731
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        dense.front_projection(**args(x0=dev['x0'].cpu()))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        dense.front_projection(**args(w1=dev['w1'].cpu()))
    with pytest.raises(RuntimeError, match='float32'):
        dense.front_projection(**args(x0=dev['x0'].double()))
    with pytest.raises(RuntimeError, match='float32'):
        dense.front_projection(**args(b1=dev['b1'].double()))
    with pytest.raises(ValueError, match='d0 = 105'):
        dense.front_projection(**args(x0=z(6, 105), x1=None, w1=z(64, 105)))
    with pytest.raises(ValueError, match='d1 = 17'):
        dense.front_projection(**args(x1=z(6, 17), w1=z(64, 33)))
    with pytest.raises(ValueError, match='dirs = 1, H = 32'):
        dense.front_projection(**args(w_ih=[z(128, 64)], b_ih=[z(128)], b_hh=[z(128)]))
    with pytest.raises(ValueError, match='at least one row'):
        dense.front_projection(**args(x0=z(0, 16), x1=z(0, 5)))
    # the C entry points, on device memory: PW_EINVAL and nothing launched
    lib, p = _lib.load(), _lib.ptr
    G, hid, big = z(6, 256), z(6, 64), z(6, 128)
    pair = lambda t: dense._pair([t])  # noqa: E731
    w_ih, b_ih, b_hh = pair(dev['w_ih'][0]), pair(dev['b_ih'][0]), pair(dev['b_hh'][0])
    stream = _lib.stream(G.device)

    def fwd(d0=16, d1=5, rows=6, dirs=1, H=64):
        return lib.pw_front_train_forward(p(big), d0, p(big), d1, p(dev['w1']), p(dev['b1']), w_ih, b_ih, b_hh, rows, dirs, H, p(hid), p(G), stream)

    def bwd(d0=16, d1=5, rows=6, dirs=1, H=64):
        out = [z(64, 128), z(64), z(256, 64), z(256)]
        scratch = z(1 << 16)
        return lib.pw_front_train_backward(p(G), p(big), d0, p(big), d1, p(hid), p(dev['w1']), w_ih, rows, dirs, H, p(out[0]), p(out[1]),
                                           pair(out[2]), pair(out[3]), None, None, p(scratch), scratch.numel() * 4, stream)
    for call in (fwd, bwd):
        for kw in (dict(d0=105), dict(d1=17), dict(dirs=1, H=32), dict(rows=0)):
            assert call(**kw) == EINVAL, (call.__name__, kw)
    torch.cuda.synchronize()
    assert float(G.abs().max()) == 0.0 and float(hid.abs().max()) == 0.0
