"""GPU: pw_head_train_forward / pw_head_train_backward and their Python surface (multiagent_rl_amd.heads: head_projection, fuse_heads,
the example learner's fused_heads switch).

Reference: tests/head_ref.py, the float64 restatement.  Bound, the project's own (tests/lstm_ref.worst_ratio <= 4): the error against
float64 is at most 4 x max(the stock float32 expression's error in the same run, one float32 rounding of the reference's largest entry).
The ReLU's mask is taken from the float32 X both sides read (with entries at +0.0, -0.0 and a tiny positive number), so float32 and
float64 agree on it by construction.
"""
import copy
import functools

import pytest
import torch

from tests import head_ref, lstm_ref, nonfinite

pytestmark = pytest.mark.gpu

# 2049 = 128 tiles of 16 rows and one row: the smallest count at which train_split gives a workgroup two tiles (129 tiles, 65
# workgroups) and the last workgroup fewer than the others (one).  6144: the length at which one summation chain failed the bound.
ROWS = (1, 15, 16, 17, 63, 65, 2049, 6144)
WIDTHS = ((1,), (5,), (16,), (1, 1), (5, 10), (5, 16), (5, 10, 21), (16, 16, 104))
EINVAL = -1


def _bits(t):
    return t.contiguous().view(torch.int32)


def _check(tag, kernel, stock, ref):
    for n in ref:
        assert n in kernel and bool(torch.isfinite(kernel[n]).all()), (tag, n)
    ratio, worst, e_k, e_s = lstm_ref.worst_ratio(kernel, stock, ref)
    print('%-66s worst %-8s kernel %.3e  stock %.3e  ratio %.2f' % (tag, worst, e_k, e_s, ratio))
    assert ratio <= 4.0, (tag, worst, e_k, e_s, ratio)
    return ratio


@functools.lru_cache(maxsize=None)
def _case(rows, widths):
    """-> (x, weights, biases on the device; the same on the CPU; dOuts float32 on the CPU); computed once and left unchanged."""
    x, ws, bs = head_ref.make_inputs(rows, widths)
    g = torch.Generator().manual_seed(rows + 7 * len(widths))
    dOuts = tuple(torch.randn(rows, n, generator=g) for n in widths)
    return (x.cuda(), [w.cuda() for w in ws], [b.cuda() for b in bs]), (x, ws, bs), dOuts


def _leaves(dev):
    leaf = lambda t: t.detach().clone().requires_grad_()  # noqa: E731
    return leaf(dev[0]), [leaf(w) for w in dev[1]], [leaf(b) for b in dev[2]]


def _named(outs, x, ws, bs):
    res = {'out%d' % k: o.detach() for k, o in enumerate(outs)}
    res['dx'] = x.grad
    for k, (w, b) in enumerate(zip(ws, bs)):
        if w.grad is not None:
            res['dW%d' % k], res['db%d' % k] = w.grad, b.grad
    return res


def _patterns(widths):
    """(name, the loss autograd sees, the dOuts it amounts to: per head a tensor or None)."""
    last, col = len(widths) - 1, min(3, widths[-1] - 1)

    def column_only(d):
        out = [None] * len(d)
        out[last] = torch.zeros_like(d[last])
        out[last][:, col] = d[last][:, col]
        return out
    pats = [('random dOut', lambda o, d: sum((a * b).sum() for a, b in zip(o, d)), lambda d: list(d)),
            ('out.sum() (expanded dOut)', lambda o, d: sum(a.sum() for a in o), lambda d: [torch.ones_like(t) for t in d]),
            ('only column %d of head %d' % (col, last), lambda o, d: (o[last][:, col] * d[last][:, col]).sum(), column_only)]
    if len(widths) > 1:
        pats.append(('only the first head used', lambda o, d: (o[0] * d[0]).sum(), lambda d: [d[0]] + [None] * (len(d) - 1)))
    return pats


# ---- 1. accuracy ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('relu', [0, 1], ids=['plain', 'relu'])
@pytest.mark.parametrize('widths', WIDTHS, ids=lambda w: 'x'.join(str(n) for n in w))
def test_head_projection_against_float64(widths, relu):
    from multiagent_rl_amd import heads
    worst = 0.0
    for rows in ROWS:
        dev, cpu, dOuts = _case(rows, widths)
        d_dev = [t.cuda() for t in dOuts]
        outs_ref = head_ref.forward(*cpu, relu)
        for name, loss, as_dOuts in _patterns(widths):
            x, ws, bs = _leaves(dev)
            outs = heads.head_projection(x, ws, bs, relu=relu)
            loss(outs, d_dev).backward()
            kernel = _named(outs, x, ws, bs)
            outs_stock, stock = head_ref.stock_grads(lambda o: loss(o, d_dev), *dev, relu)
            ref = head_ref.backward(as_dOuts(dOuts), cpu[0], cpu[1], relu)
            ref.update({'out%d' % k: o for k, o in enumerate(outs_ref)})
            stock.update({'out%d' % k: o for k, o in enumerate(outs_stock)})
            assert set(kernel) == set(ref), (name, sorted(kernel), sorted(ref))           # no gradient for a head without a dOut
            worst = max(worst, _check('rows %d widths %r relu %d %s' % (rows, widths, relu, name), kernel, stock, ref))
            if name == 'only the first head used':                                       # dX has the bits of the one-head launch
                x1, w1, b1 = _leaves((dev[0], dev[1][:1], dev[2][:1]))
                (o1,) = heads.head_projection(x1, w1, b1, relu=relu)
                (o1 * d_dev[0]).sum().backward()
                assert torch.equal(_bits(x1.grad), _bits(x.grad)) and torch.equal(_bits(w1[0].grad), _bits(ws[0].grad))
                assert torch.equal(_bits(o1), _bits(outs[0]))
    print('widths %r relu %d: worst ratio over rows and patterns %.2f' % (widths, relu, worst))


# ---- 2. determinism ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rows', [6144, 771])
def test_the_same_inputs_give_the_same_bits(rows):
    from multiagent_rl_amd import heads
    widths = (5, 10, 21)
    dev, _, dOuts = _case(rows, widths)

    def run(a, d):
        outs = heads.launch_forward(a[0], a[1], a[2], True)
        dx, dW, db = heads.launch_backward([t.cuda() for t in d], a[0], a[1], True, True)
        return outs + [dx] + dW + db
    first, second = run(dev, dOuts), run(dev, dOuts)
    other, _, other_d = _case(65, (16, 16, 104))                        # an unrelated launch of another shape in between
    run(other, other_d)
    third = run(dev, dOuts)
    for i, (a, b, c) in enumerate(zip(first, second, third)):
        assert torch.equal(_bits(a), _bits(b)) and torch.equal(_bits(a), _bits(c)), i


# ---- 3. kernel count -----------------------------------------------------------------------------------------------------------------
def _device_kernels(fn):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        out = fn()
        torch.cuda.synchronize()
    return out, [e.name for e in prof.events() if str(getattr(e, 'device_type', '')).endswith('CUDA')]


def test_one_kernel_forward_and_at_most_two_backward():
    from multiagent_rl_amd import heads
    for rows, widths, used in ((6144, (5,), (0,)), (6144, (5, 10, 21), (0, 1, 2)), (1024, (1, 1), (0,)), (16, (5, 10), (0, 1))):
        dev, _, dOuts = _case(rows, widths)
        x, ws, bs = _leaves(dev)
        leaves = [x] + ws + bs
        d = [dOuts[k].cuda() for k in used]
        grad = lambda outs: torch.autograd.grad([outs[k] for k in used], leaves, d, allow_unused=True)  # noqa: E731
        grad(heads.head_projection(x, ws, bs, relu=True))                # warm: the library is loaded, the allocator has its blocks
        torch.cuda.synchronize()
        outs, fwd = _device_kernels(lambda: heads.head_projection(x, ws, bs, relu=True))
        got, bwd = _device_kernels(lambda: grad(outs))
        print('rows %d widths %r used %r\n  forward: %r\n  backward: %r' % (rows, widths, used, fwd, bwd))
        assert len(fwd) == 1 and 'pw_head_train_forward_kernel' in fwd[0]
        assert 1 <= len(bwd) <= 2 and 'pw_head_train_backward_kernel' in bwd[0] and all('pw_head_train' in k for k in bwd)
        assert len(bwd) == (1 if rows <= 16 else 2)
        for k in range(len(widths)):                                      # an unused head: None, not zeros
            assert (got[1 + k] is not None) == (k in used) and (got[1 + len(widths) + k] is not None) == (k in used)


def _fused_pair(make):
    """The same network twice on the device, LSTM, front and (where there is one) attention fused in both; heads on in the second."""
    from multiagent_rl_amd import attention, dense, heads, lstm
    off = make().cuda()
    assert lstm.fuse_lstm(off) == 1
    attention.fuse_attention(off)
    attention.fuse_model_attention(off)
    assert dense.fuse_front(off) == 1
    on = copy.deepcopy(off)
    assert heads.fuse_heads(on) == 1 and 'fused_heads' not in off.__dict__
    return off, on


def _flat(out):
    if isinstance(out, (list, tuple)):
        return [t for o in out for t in _flat(o)]
    return [out]


NETWORKS = {
    'ActorNetwork': lambda pol, cr: pol.ActorNetwork(16, 5),
    'ActorNetwork two heads': lambda pol, cr: pol.ActorNetwork(16, [5, 3]),
    'ModelActorNetwork': lambda pol, cr: pol.ModelActorNetwork(16, 5),
    'CriticNetwork': lambda pol, cr: cr.CriticNetwork(16 + 5),
    'BiCNetCritic': lambda pol, cr: cr.BiCNetCritic(16 + 5),
    'ModelCriticNetwork': lambda pol, cr: cr.ModelCriticNetwork(16 + 5),
}


def _net_inputs(net, b, N, seed):
    g = torch.Generator().manual_seed(seed)
    obs = torch.randn(b, N, 16, generator=g)
    if hasattr(net, 'bilstm'):
        return (obs,), g
    return (obs, torch.nn.functional.one_hot(torch.randint(0, 5, (b, N), generator=g), 5).float()), g


@pytest.mark.parametrize('name', list(NETWORKS))
def test_networks_hold_fewer_kernels_with_the_switch(name):
    """Forward + backward at b = 64, N = 3.  Asserted for the one-head and the two-head ActorNetwork; printed for the others (what torch
    picks for a critic's one-column head has not been listed)."""
    from multiagent_rl_amd import critic as cr, policy as pol
    torch.manual_seed(5)
    off, on = _fused_pair(lambda: NETWORKS[name](pol, cr))
    inputs, g = _net_inputs(off, 64, 3, 1)
    inputs = [t.cuda() for t in inputs]
    weights = [torch.randn(o.shape, generator=g).cuda() for o in _flat(off(*inputs))]

    def update(net):
        for p in net.parameters():
            p.grad = None
        sum((o * w).sum() for o, w in zip(_flat(net(*inputs)), weights)).backward()
    counts = {}
    for tag, net in (('off', off), ('on', on)):
        update(net)
        torch.cuda.synchronize()
        counts[tag] = len(_device_kernels(lambda: update(net))[1])
    print('%s b 64 N 3 forward + backward: %d device kernels without the switch, %d with' % (name, counts['off'], counts['on']))
    if name in ('ActorNetwork', 'ActorNetwork two heads'):
        assert counts['on'] < counts['off'], counts


# ---- 4. non-finite inputs ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('relu', [0, 1], ids=['plain', 'relu'])
def test_non_finite_rows_stay_row_local(relu):
    """NaN, +Inf and -Inf in row 0, a mid-tile row and the last row of X (column 3) and of dOut (head 1, column 2), rows = 35: every
    output's non-finite mask is float64 autograd's of the stock expression, and clean rows keep the bits of the clean launch."""
    from multiagent_rl_amd import heads
    rows, widths = 35, (5, 10)
    dev, cpu, dOuts = _case(rows, widths)
    bad = nonfinite.rows_to_poison(rows)
    assert bad == (0, 23, 34)

    def run(x, d):
        lx, ws, bs = _leaves((x, dev[1], dev[2]))
        outs = heads.head_projection(lx, ws, bs, relu=relu)
        torch.autograd.backward(outs, [t.cuda() for t in d])
        return _named(outs, lx, ws, bs)

    def reference(x, d):
        outs, grads = head_ref.stock_grads(lambda o: sum((a * b.double()).sum() for a, b in zip(o, d)), x.double(),
                                           [w.double() for w in cpu[1]], [b.double() for b in cpu[2]], relu)
        grads.update({'out%d' % k: o for k, o in enumerate(outs)})
        return grads
    clean = run(dev[0], dOuts)
    assert all(bool(torch.isfinite(t).all()) for t in clean.values())
    for value in (nonfinite.NAN, nonfinite.INF, -nonfinite.INF):
        for where in ('X', 'dOut'):
            x, d = cpu[0], list(dOuts)
            if where == 'X':
                x = nonfinite.poisoned(x, (list(bad), 3), value)
            else:
                d[1] = nonfinite.poisoned(d[1], (list(bad), 2), value)
            got, ref = run(x.cuda(), d), reference(x, d)
            assert set(got) == set(ref)
            for n in ref:
                nonfinite.assert_same_mask(got[n], ref[n], '%s in %s, relu %d: %s' % (value, where, relu, n))
            for n in ('out0', 'out1', 'dx'):                            # the row-local outputs
                nonfinite.assert_clean_rows_same_bits(got[n], clean[n], bad, '%s in %s, relu %d: %s' % (value, where, relu, n))
            poisoned_somewhere = any(bool((~torch.isfinite(t)).any()) for t in got.values())
            assert poisoned_somewhere or (relu and where == 'X' and value == -nonfinite.INF)     # relu(-Inf) = 0 poisons nothing


# ---- 5. the six networks -------------------------------------------------------------------------------------------------------------
def _outputs_and_grads(net, inputs, weights):
    for p in net.parameters():
        p.grad = None
    outs = _flat(net(*inputs))
    sum((o * w.to(o)).sum() for o, w in zip(outs, weights)).backward()
    res = {'out%d' % i: o.detach() for i, o in enumerate(outs)}
    res.update({n: p.grad.detach().clone() for n, p in net.named_parameters()})
    return res


@pytest.mark.parametrize('name', list(NETWORKS))
def test_networks_with_the_switch_against_float64(name):
    from multiagent_rl_amd import critic as cr, heads, policy as pol
    torch.manual_seed(11)
    plain = NETWORKS[name](pol, cr)
    ref_net = copy.deepcopy(plain).double()
    off, on = _fused_pair(lambda: copy.deepcopy(plain))
    b = 257
    for N in (1, 3, 6):
        inputs, g = _net_inputs(plain, b, N, N)
        outs = _flat(ref_net(*[t.double() for t in inputs]))
        weights = [torch.randn(o.shape, generator=g) for o in outs]
        ref = _outputs_and_grads(ref_net, [t.double() for t in inputs], weights)
        dev_in = [t.cuda() for t in inputs]
        _check('%s b %d N %d' % (name, b, N), _outputs_and_grads(on, dev_in, weights), _outputs_and_grads(off, dev_in, weights), ref)
    assert list(on.state_dict()) == list(off.state_dict()) == list(plain.state_dict())
    assert heads.unfuse_heads(on) == 1
    again, stock = _outputs_and_grads(on, dev_in, weights), _outputs_and_grads(off, dev_in, weights)
    assert all(torch.equal(_bits(again[n]), _bits(stock[n])) for n in stock)        # switched off: the stock calls, bit for bit


# ---- 6. the capability: graphed and eager updates with the fused heads, bit for bit --------------------------------------------------
def _learner(ug, variant, nets, graph, heads=True):
    import madr_learner
    from multiagent_rl_amd.policy import accelerate_trainer
    cls_name, _, _, ring_kw, N, D = ug.VARIANTS[variant]
    actor, critic = copy.deepcopy(nets)
    t = getattr(madr_learner, cls_name)(actor, critic, ug._filled_memory(ring_kw, N, D),
                                        action_type='MultiDiscrete' if 'act_heads' in ring_kw else 'Discrete', batch_size=64,
                                        fused_optimizer=True, fused_lstm=True, fused_attention=True, graph_update=graph,
                                        fused_sampling=True, sampling_seed=5, fused_front=True, fused_wgrad=True, fused_heads=heads)
    if not graph:
        accelerate_trainer(t, targets=True)
    return t


@pytest.mark.parametrize('variant', ['attention', 'two_head', 'bicnet', 'model'])
def test_graphed_updates_with_the_fused_heads_equal_eager_updates_bit_for_bit(variant):
    """Learners A and B eager, C graphed, all with fused_heads and every other switch: A == B == C in every parameter, target, Adam
    moment and loss after each of 8 updates and after a learning-rate change (a re-capture).  Learner D, without the switch, starts
    from the same weights: after the first update both losses agree with A's to 1e-3 relative (one update from identical weights: only
    the summation order differs)."""
    import tests.test_gpu_update_graph as ug                              # the harness: VARIANTS, _filled_memory, _everything, _same
    from multiagent_rl_amd import critic as cr, policy as pol
    from multiagent_rl_amd.graph import GraphedUpdate
    torch.manual_seed(3)
    nets = (ug.VARIANTS[variant][1](pol, cr), ug.VARIANTS[variant][2](pol, cr))
    a, b, c = (_learner(ug, variant, nets, graph) for graph in (False, False, True))
    d = _learner(ug, variant, nets, False, heads=False)
    assert isinstance(c.optimize, GraphedUpdate)
    for t in (a, b, c):
        assert t.actor.fused_heads and t.critic.fused_heads
    assert a.target_actor.fused_heads and a.target_critic.fused_heads      # the deep copies carry it (read through the target wrappers)
    assert 'fused_heads' not in d.actor.__dict__ and 'fused_heads' not in d.critic.__dict__

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
    g = c.optimize
    assert (g.eager_calls, g.captures, g.replays) == (3, 1, 5)
    for t in (a, c):                                                       # a changed learning rate: captured again, still the eager learner's bits
        for opt in (t.actor_optimizer, t.critic_optimizer):
            opt.param_groups[0]['lr'] = 1e-3
    la, lc = step(a, 0), step(c, 2)
    assert g.captures == 2 and la == lc and all(ug._same(x, y) for x, y in zip(ug._everything(a), ug._everything(c)))


def test_accelerate_trainer_heads_switch():
    """heads=True needs swapped networks (its own front=True counts) and reaches the target networks that are still modules."""
    import madr_learner
    import tests.test_gpu_update_graph as ug
    from multiagent_rl_amd import critic as cr, policy as pol
    _, mk_actor, mk_critic, ring_kw, N, D = ug.VARIANTS['attention']
    make = lambda **kw: madr_learner.Trainer(mk_actor(pol, cr), mk_critic(pol, cr), ug._filled_memory(ring_kw, N, D), batch_size=ug.BATCH, **kw)  # noqa: E731
    with pytest.raises(ValueError, match='front=True'):
        pol.accelerate_trainer(make(fused_lstm=True), heads=True)
    t = make()
    fx = pol.accelerate_trainer(t, lstm=True, attention=True, front=True, heads=True)
    assert fx.fused_heads == 4 and all(n.fused_heads for n in (t.actor, t.critic, t.target_actor, t.target_critic))
    la, lc = t.optimize()
    assert la == la and lc == lc
    t = make(fused_lstm=True, fused_front=True)
    fx = pol.accelerate_trainer(t, targets=True, heads=True)               # the targets are wrappers on the no-gradient kernels: left alone
    assert fx.fused_heads == 2 and t.critic.fused_heads


# ---- 7. refusals on the device -------------------------------------------------------------------------------------------------------
def test_refusals_on_the_device():
    from multiagent_rl_amd import _lib, heads
    dev, _, _ = _case(17, (5, 10))
    x, ws, bs = dev
    z = lambda *s: torch.zeros(*s, device='cuda')  # noqa: E731
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        heads.head_projection(x.cpu(), ws, bs)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        heads.head_projection(x, [ws[0].cpu(), ws[1]], bs)
    with pytest.raises(RuntimeError, match='float32'):
        heads.head_projection(x.double(), ws, bs)
    with pytest.raises(ValueError, match='105 columns wide'):
        heads.head_projection(x, [z(105, 64)], [z(105)])
    # the C entry points, on device memory: PW_EINVAL and nothing launched
    lib, p = _lib.load(), _lib.ptr
    outs, dx = [z(17, 5), z(17, 10)], z(17, 64)
    dW, db, scratch = [z(5, 64), z(10, 64)], [z(5), z(10)], z(1 << 14)
    stream = _lib.stream(x.device)

    def fwd(rows=17, heads_=2, n=(5, 10)):
        return lib.pw_head_train_forward(p(x), rows, 1, heads_, heads._pointers(ws), heads._pointers(bs), heads._widths(n), heads._pointers(outs), stream)

    def bwd(rows=17, heads_=2, n=(5, 10), dOut=None, dW_=None):
        return lib.pw_head_train_backward(heads._pointers(outs if dOut is None else dOut), p(x), rows, 1, heads_, heads._pointers(ws),
                                          heads._widths(n), p(dx), heads._pointers(dW if dW_ is None else dW_), heads._pointers(db), p(scratch),
                                          scratch.numel() * 4, stream)
    for call in (fwd, bwd):
        for kw in (dict(rows=0), dict(heads_=0), dict(heads_=4), dict(n=(5, 105)), dict(n=(0, 10))):
            assert call(**kw) == EINVAL, (call.__name__, kw)
    assert bwd(dOut=[None, None], dW_=[None, None]) == EINVAL and bwd(dOut=[outs[0], None]) == EINVAL
    torch.cuda.synchronize()
    assert all(float(t.abs().max()) == 0.0 for t in outs + dW + db + [dx])
