"""GPU: pw_adam_step (global-norm clip + Adam + Polyak update, one launch) and pw_soft_update, and their Python surface
(multiagent_rl_amd.optim, accelerate_trainer(optimizer=True)).

(a) Parameter sets: a two-head ActorNetwork(21, [5, 10]) and a CriticNetwork(16 + 5) moved to the GPU (their LSTM tensors are
    what .cuda() leaves: views of one flat buffer where the RNN backend flattens); a synthetic set with numel in
    {1, 3, 5, 63, 64, 65, 1027, 16385} of which two tensors start one element into a larger storage (4-byte aligned only);
    a set of exactly 32 tensors.
(b) 25 steps of fresh random gradients from one float32 start, at gradient scales x1e-3 / x1 / x30 (max_norm 0.5: never clipped
    at x1e-3, coef between 3e-3 and 0.1 at x1, 30 times smaller at x30; a nine-element case has norms on both sides of
    max_norm).  In the same run: the kernel's worst |dp|, |dexp_avg|, |dexp_avg_sq| against
    the float64 restatement (tests/optim_ref.py), and those of stock float32 clip_grad_norm_ + torch.optim.Adam(foreach=False)
    on the GPU.  Bound, per quantity: kernel <= 4 x stock (a different but equally long rounding chain).  total_norm within
    2e-6 relative of float64 at every step ((log2 n + 2) * 2^-24 for a tree sum of n <= 2^20 positive terms).
(c) Soft update: bit-identical to torch's `t * (1.0 - tau) + p * tau` on the GPU for tau in {1e-2, 0.5}; tau = 1 copies, also over
    an infinity; the target written by pw_adam_step equals the standalone update applied to that launch's new parameters.
(d) Two runs from one state give the same bits; a parameter without gradient keeps value and state and stays out of the norm
    (its target still moves); a NaN gradient spreads as clip_grad_norm_ spreads it; a second stream works; what FusedAdam refuses.
(e) accelerate_trainer(optimizer=True) on a stand-in Trainer with real backward passes: see test_accelerate_trainer_optimizer;
    the fused_optimizer switch of examples/madr_learner.py and examples/train_batched.py --fused-optimizer.

``PW_OPTIM_F64_REPORT=<path>``: every case appends its figures there (profiles/optimizer_vs_f64.txt is where such a run is kept).
"""
import copy
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

from tests import optim_ref  # noqa: E402

LR, BETAS, EPS, MAX_NORM, STEPS = 1e-2, (0.9, 0.999), 1e-8, 0.5, 25
GAMMA, TAU = 0.95, 1e-2
SETS = ['actor', 'critic', 'synthetic', 'exact32']
SCALES = [1e-3, 1.0, 30.0]
SYNTHETIC = [1, 3, 5, 63, 64, 65, 1027, 16384 + 1]


def _report(line):
    print(line)
    path = os.environ.get('PW_OPTIM_F64_REPORT')
    if path:
        with open(path, 'a') as f:
            f.write(line + '\n')


def _offset_view(values, lead):
    """A leaf tensor that starts ``lead`` elements into a larger storage."""
    big = torch.zeros(values.numel() + lead + 2, device='cuda')
    view = big[lead:lead + values.numel()].view(values.shape).detach()
    view.copy_(values)
    return view


def _param_set(name, seed=0):
    """-> list of leaf float32 GPU tensors (requires_grad), freshly built from ``seed``: two calls give equal, independent sets."""
    torch.manual_seed(seed)
    if name == 'actor':
        from multiagent_rl_amd.policy import ActorNetwork
        return list(ActorNetwork(21, [5, 10]).cuda().parameters())
    if name == 'critic':
        from multiagent_rl_amd.critic import CriticNetwork
        return list(CriticNetwork(16 + 5, 1).cuda().parameters())
    g = torch.Generator().manual_seed(seed + 17)
    if name == 'synthetic':
        out = []
        for i, n in enumerate(SYNTHETIC):
            v = (torch.randn(n, generator=g) * 0.1).cuda()
            out.append((_offset_view(v, 1) if n in (65, 1027) else v).requires_grad_())
        return out
    assert name == 'exact32'
    return [(torch.randn(1 + (7 * i) % 97, generator=g) * 0.1).cuda().requires_grad_() for i in range(32)]


def _grads(params, rng, scale, misalign=False):
    out = []
    for i, p in enumerate(params):
        g = torch.from_numpy((rng.standard_normal(tuple(p.shape)) * scale).astype(np.float32)).cuda()
        out.append(_offset_view(g, 3) if (misalign and i % 3 == 1) else g)
    return out


def _np(ts):
    return [t.detach().cpu().numpy().astype(np.float64) for t in ts]


def _worst(xs, ys):
    return max(float(np.abs(x - y).max()) for x, y in zip(xs, ys))


_cache = {}


def _measure(name, scale):
    """The 25-step run of (b) for one set and scale -> dict of worst errors (kernel / stock, against float64) and the norms."""
    key = (name, scale)
    if key in _cache:
        return _cache[key]
    from multiagent_rl_amd.optim import FusedAdam
    pk, ps = _param_set(name), _param_set(name)
    assert all(torch.equal(a, b) for a, b in zip(pk, ps)) and len(pk) <= 32
    fused = FusedAdam(pk, lr=LR, betas=BETAS, eps=EPS, max_norm=MAX_NORM)
    stock = torch.optim.Adam(ps, lr=LR, betas=BETAS, eps=EPS, foreach=False)
    ref = optim_ref.AdamF64(_np(pk), lr=LR, betas=BETAS, eps=EPS, max_norm=MAX_NORM)
    rng = np.random.RandomState(len(pk) * 1000 + int(scale * 7))
    norms_k, norms_64, coefs = [], [], []
    for it in range(STEPS):
        gs = _grads(pk, rng, scale, misalign=(name == 'synthetic'))
        keep = [g.clone() for g in gs]
        for p, q, g in zip(pk, ps, gs):
            p.grad, q.grad = g, g.clone()
        fused.step()
        norms_k.append(fused.last_total_norm.clone())
        assert all(torch.equal(_bits(p.grad), _bits(g)) for p, g in zip(pk, keep))    # gradients are read, never written
        del keep
        torch.nn.utils.clip_grad_norm_(ps, MAX_NORM, foreach=False)
        stock.step()
        ref.step([g.cpu().numpy() for g in gs])
        norms_64.append(ref.total_norm)
        coefs.append(min(1.0, MAX_NORM / (ref.total_norm + 1e-6)))
    res = dict(
        kernel=(_worst(_np(pk), ref.p), _worst(_np([fused.state[p]['exp_avg'] for p in pk]), ref.m),
                _worst(_np([fused.state[p]['exp_avg_sq'] for p in pk]), ref.v)),
        stock=(_worst(_np(ps), ref.p), _worst(_np([stock.state[p]['exp_avg'] for p in ps]), ref.m),
               _worst(_np([stock.state[p]['exp_avg_sq'] for p in ps]), ref.v)),
        norm_rel=max(abs(float(a) - b) / b for a, b in zip(norms_k, norms_64)),
        coef=(min(coefs), max(coefs)), steps=[float(fused.state[p]['step']) for p in pk],
        flat=sum(1 for p in pk if p.data_ptr() % 16), tensors=len(pk), numel=sum(p.numel() for p in pk))
    _cache[key] = res
    return res


@pytest.mark.parametrize('scale', SCALES, ids=lambda s: 'x%g' % s)
@pytest.mark.parametrize('name', SETS)
def test_accuracy_against_float64_within_4x_of_stock_float32(name, scale):
    r = _measure(name, scale)
    ratios = [k / s if s > 0 else (0.0 if k == 0 else float('inf')) for k, s in zip(r['kernel'], r['stock'])]
    _report('%-9s x%-5g %2d tensors %6d elements (%d not 16-byte aligned)  coef %.3g..%.3g | kernel |dp| %.2e |dm| %.2e |dv| %.2e | '
            'stock f32 %.2e %.2e %.2e | ratio %.2f %.2f %.2f | total_norm rel %.1e' % (
                name, scale, r['tensors'], r['numel'], r['flat'], r['coef'][0], r['coef'][1], *r['kernel'], *r['stock'], *ratios,
                r['norm_rel']))
    assert r['steps'] == [float(STEPS)] * r['tensors']
    if scale == 1e-3:
        assert r['coef'][0] == 1.0                                   # never clipped
    if scale == 30.0:
        assert r['coef'][1] < 1.0                                    # always clipped
    assert r['norm_rel'] <= 2e-6, r['norm_rel']
    for what, k, s in zip(('param', 'exp_avg', 'exp_avg_sq'), r['kernel'], r['stock']):
        assert k <= 4.0 * s, '%s x%g %s: kernel %.3g against float64, stock float32 %.3g (bound 4 x)' % (name, scale, what, k, s)


def test_norms_on_both_sides_of_max_norm():
    """Nine elements at scale 0.17: the norm lands on either side of max_norm from step to step (the clip is active in some steps
    only).  Norm, p, exp_avg and exp_avg_sq against float64, the latter three within 4 x stock float32 as in (b)."""
    rng = np.random.RandomState(1)
    from multiagent_rl_amd.optim import FusedAdam
    pk, ps = _param_set('synthetic')[:3], _param_set('synthetic')[:3]   # 9 elements: |g| straddles 0.5 from step to step
    fused = FusedAdam(pk, lr=LR, max_norm=MAX_NORM)
    stock = torch.optim.Adam(ps, lr=LR, foreach=False)
    ref = optim_ref.AdamF64(_np(pk), lr=LR, max_norm=MAX_NORM)
    seen = set()
    for _ in range(STEPS):
        gs = _grads(pk, rng, 0.17)
        for p, q, g in zip(pk, ps, gs):
            p.grad, q.grad = g, g.clone()
        fused.step()
        torch.nn.utils.clip_grad_norm_(ps, MAX_NORM, foreach=False)
        stock.step()
        ref.step([g.cpu().numpy() for g in gs])
        assert abs(float(fused.last_total_norm) - ref.total_norm) <= 2e-6 * ref.total_norm
        seen.add(ref.total_norm > MAX_NORM)
    assert seen == {True, False}
    kernel = (_worst(_np(pk), ref.p), _worst(_np([fused.state[p]['exp_avg'] for p in pk]), ref.m),
              _worst(_np([fused.state[p]['exp_avg_sq'] for p in pk]), ref.v))
    base = (_worst(_np(ps), ref.p), _worst(_np([stock.state[p]['exp_avg'] for p in ps]), ref.m),
            _worst(_np([stock.state[p]['exp_avg_sq'] for p in ps]), ref.v))
    _report('nine elements, clip active in some steps: kernel |dp| %.2e |dm| %.2e |dv| %.2e | stock f32 %.2e %.2e %.2e' % (*kernel, *base))
    for what, k, s in zip(('param', 'exp_avg', 'exp_avg_sq'), kernel, base):
        assert k <= 4.0 * s, '%s: kernel %.3g against float64, stock float32 %.3g (bound 4 x)' % (what, k, s)


def test_a_nan_gradient_reaches_every_element_of_a_clipping_call():
    """clip_grad_norm_ multiplies every gradient by its NaN coefficient; the kernel's coef does the same.  Without a clip the NaN
    stays in its own element."""
    from multiagent_rl_amd.optim import FusedAdam
    for max_norm in (MAX_NORM, None):
        pk, ps = _param_set('synthetic')[:4], _param_set('synthetic')[:4]
        fused, stock = FusedAdam(pk, lr=LR, max_norm=max_norm), torch.optim.Adam(ps, lr=LR, foreach=False)
        for p, q in zip(pk, ps):
            p.grad, q.grad = torch.ones_like(p), torch.ones_like(q)
        pk[1].grad[2] = ps[1].grad[2] = float('nan')
        fused.step()
        if max_norm is not None:
            torch.nn.utils.clip_grad_norm_(ps, max_norm, foreach=False)
        stock.step()
        assert bool(torch.isnan(fused.last_total_norm))
        for p, q in zip(pk, ps):
            assert torch.equal(torch.isnan(p), torch.isnan(q))
        assert bool(torch.isnan(pk[0]).all()) == (max_norm is not None) and bool(torch.isnan(pk[1][2]))


def test_weight_decay_and_plain_adam_against_float64():
    """weight_decay (L2 form, after the clip) and the launch without clip and without norm output."""
    from multiagent_rl_amd.optim import FusedAdam
    for wd, max_norm in ((1e-2, MAX_NORM), (0.0, None), (0.3, None)):
        pk, ps = _param_set('synthetic'), _param_set('synthetic')
        fused = FusedAdam(pk, lr=LR, weight_decay=wd, max_norm=max_norm)
        stock = torch.optim.Adam(ps, lr=LR, weight_decay=wd, foreach=False)
        ref = optim_ref.AdamF64(_np(pk), lr=LR, weight_decay=wd, max_norm=max_norm)
        rng = np.random.RandomState(4)
        for it in range(STEPS):
            gs = _grads(pk, rng, 3.0)
            for p, q, g in zip(pk, ps, gs):
                p.grad, q.grad = g, g.clone()
            fused.step()
            if max_norm is not None:
                torch.nn.utils.clip_grad_norm_(ps, max_norm, foreach=False)
            stock.step()
            ref.step([g.cpu().numpy() for g in gs])
        k, s = _worst(_np(pk), ref.p), _worst(_np(ps), ref.p)
        _report('synthetic wd %g max_norm %s: kernel |dp| %.2e  stock f32 %.2e  ratio %.2f' % (wd, max_norm, k, s, k / s))
        assert k <= 4.0 * s, (wd, max_norm, k, s)


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


@pytest.mark.parametrize('tau', [1e-2, 0.5])
@pytest.mark.parametrize('name', ['actor', 'critic', 'synthetic', 'exact32'])
def test_soft_update_is_torchs_expression_bit_for_bit(name, tau):
    from multiagent_rl_amd.optim import soft_update
    target, source = _param_set(name, seed=1), _param_set(name, seed=2)
    want = [t.data * (1.0 - tau) + s.data * tau for t, s in zip(target, source)]           # ddpg_gumbel_fix.py:44-47
    keep = [s.detach().clone() for s in source]
    soft_update(target, source, tau)
    for t, w, s, k in zip(target, want, source, keep):
        assert torch.equal(_bits(t), _bits(w)), (name, tau, tuple(t.shape), int((_bits(t) != _bits(w)).sum()))
        assert torch.equal(_bits(s), _bits(k))
    host = optim_ref.soft_update_f32(_param_set(name, seed=1)[-1].detach().cpu().numpy(), keep[-1].cpu().numpy(), tau)
    assert np.array_equal(host.view(np.uint32), target[-1].detach().cpu().numpy().view(np.uint32))


def test_soft_update_on_modules_and_tau_one_copies_over_infinity():
    from multiagent_rl_amd.critic import CriticNetwork, _FusedTarget
    from multiagent_rl_amd.optim import soft_update
    torch.manual_seed(1)
    target, source = CriticNetwork(21, 1).cuda(), CriticNetwork(21, 1).cuda()
    want = [t.data * (1.0 - TAU) + s.data * TAU for t, s in zip(target.parameters(), source.parameters())]
    soft_update(_FusedTarget(target, None), source, TAU)                                  # the wrapper of accelerate_trainer(targets=True)
    assert all(torch.equal(_bits(t), _bits(w)) for t, w in zip(target.parameters(), want))
    with torch.no_grad():
        for p in target.parameters():
            p.view(-1)[0] = float('inf')
            p.view(-1)[-1] = float('-inf')
    soft_update(target, source, 1.0)                                                     # hard_update: inf * 0 must not appear
    assert all(torch.equal(_bits(t), _bits(s)) for t, s in zip(target.parameters(), source.parameters()))
    t = [torch.full((5,), float('inf'), device='cuda')]
    soft_update(t, [torch.ones(5, device='cuda')], 0.5)
    assert bool(torch.isinf(t[0]).all())                                                 # below tau = 1 the expression is torch's: inf stays


@pytest.mark.parametrize('tau', [1e-2, 0.5, 1.0])
def test_fused_target_equals_standalone_soft_update_of_the_new_parameters(tau):
    from multiagent_rl_amd.optim import FusedAdam, soft_update
    for name in ('critic', 'synthetic'):
        params, plain = _param_set(name), _param_set(name)
        targets = [t.detach() for t in _param_set(name, seed=5)]
        old = [t.clone() for t in targets]
        fused = FusedAdam(params, lr=LR, max_norm=MAX_NORM, targets=targets, tau=tau)
        alone = FusedAdam(plain, lr=LR, max_norm=MAX_NORM)
        rng = np.random.RandomState(2)
        for it in range(3):
            gs = _grads(params, rng, 1.0)
            for p, q, g in zip(params, plain, gs):
                p.grad, q.grad = g, g
            fused.step()
            alone.step()
            soft_update(old, plain, tau)
            for p, q, t, o in zip(params, plain, targets, old):
                assert torch.equal(_bits(p), _bits(q))                                   # the soft update does not touch the Adam step
                assert torch.equal(_bits(t), _bits(o)), (name, tau, it)
        assert torch.equal(_bits(fused.last_total_norm), _bits(alone.last_total_norm))


def _run(name, skip=None, stream=None, steps=4):
    from multiagent_rl_amd.optim import FusedAdam
    params = _param_set(name)
    targets = [t.detach() for t in _param_set(name, seed=5)]
    opt = FusedAdam(params, lr=LR, max_norm=MAX_NORM, targets=targets, tau=TAU)
    rng = np.random.RandomState(8)
    norms = []
    for it in range(steps):
        gs = _grads(params, rng, 1.0)
        for i, (p, g) in enumerate(zip(params, gs)):
            p.grad = None if i == skip else g
        if stream is None:
            opt.step()
        else:
            torch.cuda.synchronize()
            with torch.cuda.stream(stream):
                opt.step()
            stream.synchronize()
        norms.append(opt.last_total_norm.clone())
    return params, targets, opt, norms, gs


def test_two_runs_give_the_same_bits_and_a_second_stream_works():
    for name in ('actor', 'synthetic'):
        a, b = _run(name), _run(name)
        c = _run(name, stream=torch.cuda.Stream())
        for other in (b, c):
            for x, y in zip(a[0] + a[1] + a[3], other[0] + other[1] + other[3]):
                assert torch.equal(_bits(x), _bits(y)), name
            for p, q in zip(a[0], other[0]):
                for k in ('exp_avg', 'exp_avg_sq'):
                    assert torch.equal(_bits(a[2].state[p][k]), _bits(other[2].state[q][k])), (name, k)


def test_a_parameter_without_gradient_takes_no_part():
    skip = 6                                                         # the 1027-element tensor of the synthetic set
    start, start_t = _param_set('synthetic'), _param_set('synthetic', seed=5)
    params, targets, opt, norms, gs = _run('synthetic', skip=skip, steps=2)
    assert torch.equal(_bits(params[skip]), _bits(start[skip]))
    want = start_t[skip].detach()                                    # its target still moves, as the stock soft_update moves every target
    for _ in range(2):
        want = want * (1.0 - TAU) + start[skip].detach() * TAU
    assert torch.equal(_bits(targets[skip]), _bits(want))
    assert len(opt.state[params[skip]]) == 0                         # no state was created, as in torch
    assert all(float(opt.state[p]['step']) == 2.0 for i, p in enumerate(params) if i != skip)
    n64 = float(np.sqrt(sum(float((g.double() ** 2).sum()) for i, g in enumerate(gs) if i != skip)))
    assert abs(float(norms[-1]) - n64) <= 2e-6 * n64
    assert not torch.equal(_bits(params[0]), _bits(start[0]))
    # it joins later: its own step count then disagrees with the group's, which one launch cannot serve
    params[skip].grad = gs[skip]
    with pytest.raises(RuntimeError, match='step'):
        opt.step()


def test_what_fused_adam_refuses_on_the_gpu():
    from multiagent_rl_amd.optim import FusedAdam

    def one_step(params, grads=None):
        params = [p.requires_grad_() for p in params]
        for i, p in enumerate(params):
            p.grad = torch.ones_like(p) if grads is None else grads[i]
        FusedAdam(params, lr=LR).step()
    with pytest.raises(RuntimeError, match='float32'):
        one_step([torch.zeros(8, device='cuda', dtype=torch.float64)])
    with pytest.raises(RuntimeError, match='contiguous'):
        one_step([torch.zeros(8, 6, device='cuda').t()])
    with pytest.raises(RuntimeError, match='sparse'):
        one_step([torch.zeros(8, 6, device='cuda')], [torch.zeros(8, 6, device='cuda').to_sparse()])
    with pytest.raises(RuntimeError, match='32 tensors'):
        one_step([torch.zeros(2, device='cuda') for _ in range(33)])
    with pytest.raises(RuntimeError, match='2\\^20'):
        one_step([torch.zeros(1 << 19, device='cuda'), torch.zeros((1 << 19) + 1, device='cuda')])
    one_step([torch.zeros(1 << 19, device='cuda'), torch.zeros(1 << 19, device='cuda')])     # exactly 2^20 elements: served
    torch.cuda.synchronize()


def test_full_size_call_matches_float64():
    """2^20 elements in one call (513 workgroups, each summing every gradient): one clipped step against float64."""
    from multiagent_rl_amd.optim import FusedAdam
    g = torch.Generator().manual_seed(3)
    params = [(torch.randn(n, generator=g) * 0.1).cuda().requires_grad_() for n in ((1 << 20) - 4099, 4099)]
    grads = [torch.randn(p.shape, generator=g).cuda() for p in params]
    ref = optim_ref.AdamF64(_np(params), lr=LR, max_norm=MAX_NORM)
    for p, gr in zip(params, grads):
        p.grad = gr
    opt = FusedAdam(params, lr=LR, max_norm=MAX_NORM)
    opt.step()
    ref.step([x.cpu().numpy() for x in grads])
    assert abs(float(opt.last_total_norm) - ref.total_norm) <= 2e-6 * ref.total_norm
    # one step from zero state: p - lr * g / (|g| + eps'), every operation correctly rounded: a few ulp of |p| <= 0.6
    assert _worst(_np(params), ref.p) <= 4 * 2.0 ** -24


class _StandInTrainer(object):
    """The surface of the reference's Trainer that accelerate_trainer touches, written for this test (the pattern of
    tests/test_gpu_critic.py's stand-in, with real losses): targets as deep copies, Adam optimisers, soft_update / hard_update over
    parameters(), an optimize() in the order of ddpg_gumbel_fix.py:145-213 -- TD target from the target networks, critic loss,
    backward, clip_grad_norm_(0.5), step; actor loss through the critic, backward, clip, step; two soft updates -- and
    save / load through state_dict()."""

    def __init__(self, actor, critic, out_dir):
        self.device = torch.device('cuda', torch.cuda.current_device())
        self.actor, self.critic = actor.to(self.device), critic.to(self.device)
        self.target_actor, self.target_critic = copy.deepcopy(self.actor), copy.deepcopy(self.critic)
        self.target_actor.eval()
        self.target_critic.eval()
        self.actor_optimizer = torch.optim.Adam(self.actor.parameters(), LR)
        self.critic_optimizer = torch.optim.Adam(self.critic.parameters(), LR)
        self.action_type, self.out_dir, self.batch = 'Discrete', out_dir, None

    def soft_update(self, target, source, tau):
        for tp, sp in zip(target.parameters(), source.parameters()):
            tp.data.copy_(tp.data * (1.0 - tau) + sp.data * tau)

    def hard_update(self, target, source):
        for tp, sp in zip(target.parameters(), source.parameters()):
            tp.data.copy_(sp.data)

    def gumbel_softmax(self, x):
        n, t = x.size(0), x.size(1)
        y = torch.nn.functional.gumbel_softmax(x.contiguous().view(n * t, x.size(2)), hard=True)
        return y.contiguous().view(n, t, -1)

    def optimize(self):
        s0, a0, r, s1, d = self.batch
        a1 = self.gumbel_softmax(self.target_actor.forward(s1))
        q_next = torch.squeeze(self.target_critic.forward(s1, a1).detach())
        y = r + GAMMA * q_next * (1. - d)
        loss_critic = torch.nn.SmoothL1Loss()(torch.squeeze(self.critic.forward(s0, a0)), y)
        self.critic_optimizer.zero_grad()
        loss_critic.backward()
        torch.nn.utils.clip_grad_norm_(self.critic.parameters(), 0.5)
        self.critic_optimizer.step()
        loss_actor = -1 * self.critic.forward(s0, self.gumbel_softmax(self.actor.forward(s0))).mean()
        self.actor_optimizer.zero_grad()
        loss_actor.backward()
        torch.nn.utils.clip_grad_norm_(self.actor.parameters(), 0.5)
        self.actor_optimizer.step()
        self.soft_update(self.target_actor, self.actor, TAU)
        self.soft_update(self.target_critic, self.critic, TAU)
        return loss_actor.detach(), loss_critic.detach()

    def save_models(self, fname):
        torch.save(self.target_actor.state_dict(), os.path.join(self.out_dir, fname + '_actor.pt'))
        torch.save(self.target_critic.state_dict(), os.path.join(self.out_dir, fname + '_critic.pt'))

    def load_models(self, fname):
        self.actor.load_state_dict(torch.load(os.path.join(self.out_dir, fname + '_actor.pt')))
        self.critic.load_state_dict(torch.load(os.path.join(self.out_dir, fname + '_critic.pt')))
        self.hard_update(self.target_actor, self.actor)
        self.hard_update(self.target_critic, self.critic)


def _trainer(tmp_path, warm=2):
    """A stand-in Trainer that has already taken ``warm`` stock updates (so that the optimisers it hands over hold state)."""
    from multiagent_rl_amd.critic import CriticNetwork
    from multiagent_rl_amd.policy import ActorNetwork
    torch.manual_seed(11)
    tr = _StandInTrainer(ActorNetwork(16, 5), CriticNetwork(21, 1), str(tmp_path))
    g = torch.Generator().manual_seed(4)
    for it in range(warm):
        tr.batch = _batch(g)
        torch.manual_seed(50 + it)
        tr.optimize()
    return tr


def _batch(g, b=1024, N=6, D=16, A=5):
    a0 = torch.nn.functional.one_hot(torch.randint(0, A, (b, N), generator=g), A).float()
    return ((torch.randn(b, N, D, generator=g) * 2).cuda(), a0.cuda(), (torch.randn(b, generator=g) * 3).cuda(),
            (torch.randn(b, N, D, generator=g) * 2).cuda(), (torch.rand(b, generator=g) < 0.2).float().cuda())


def _nets(tr):
    mods = (tr.actor, tr.critic, getattr(tr.target_actor, 'module', tr.target_actor), getattr(tr.target_critic, 'module', tr.target_critic))
    return [list(m.parameters()) for m in mods]


@pytest.mark.parametrize('targets', [False, True], ids=['optimizer', 'targets+optimizer'])
def test_accelerate_trainer_optimizer(tmp_path, targets):
    """Three optimize() calls of the patched Trainer against the same Trainer with stock optimisers and soft updates, same seeds,
    gradients from stock autograd in both.  Bound: both optimisers are within their (b) error of float64 Adam, the kernel's being
    at most 4 x the stock one e, so the two differ by at most 5 e, with e = stock float32's worst |dp| against float64 measured
    in (b) on the actor and critic sets at scale x1 and this learning rate (25 steps there, 3 here).  The targets move by tau of
    that.  With targets=True the baseline has targets=True as well: the fused target networks change y by design (2e-5, and
    another sampled a1 on a few rows -- tests/test_gpu_critic.py), which is not the optimiser's doing and which Adam's
    normalisation would carry into the parameters at the size of the learning rate."""
    from multiagent_rl_amd.critic import CriticNetwork, accelerate_trainer
    from multiagent_rl_amd.optim import FusedAdam
    from multiagent_rl_amd.policy import ActorNetwork
    e = max(_measure('actor', 1.0)['stock'][0], _measure('critic', 1.0)['stock'][0])
    bound = 5.0 * e
    plain, fused = _trainer(tmp_path), _trainer(tmp_path)
    for a, b in zip(sum(_nets(plain), []), sum(_nets(fused), [])):
        assert torch.equal(a, b)
    old_state = copy.deepcopy(fused.critic_optimizer.state_dict())
    soft0 = fused.soft_update
    accelerate_trainer(fused, seed=3)                                   # the default leaves optimisers and soft_update alone
    assert type(fused.actor_optimizer) is torch.optim.Adam and fused.soft_update == soft0
    if targets:
        accelerate_trainer(plain, seed=3, targets=True)
    accelerate_trainer(fused, seed=3, targets=targets, optimizer=True)
    assert isinstance(fused.actor_optimizer, FusedAdam) and isinstance(fused.critic_optimizer, FusedAdam)
    assert fused.critic_optimizer.max_norm is None and fused.critic_optimizer.param_groups[0]['lr'] == LR
    new_state = fused.critic_optimizer.state_dict()
    assert float(new_state['state'][0]['step']) == 2.0 and torch.equal(new_state['state'][3]['exp_avg'], old_state['state'][3]['exp_avg'])
    assert (type(fused.target_critic).__name__ == '_FusedTarget') == targets
    g = torch.Generator().manual_seed(5)
    for it in range(3):
        plain.batch = fused.batch = _batch(g)
        torch.manual_seed(100 + it)
        lp = plain.optimize()
        torch.manual_seed(100 + it)
        lf = fused.optimize()
        assert all(bool(torch.isfinite(x)) for x in lp + lf)
    worst = [max(float((a - b).detach().abs().max()) for a, b in zip(x, y)) for x, y in zip(_nets(plain), _nets(fused))]
    _report('accelerate_trainer(targets=%s, optimizer=True), 3 optimize(): |d actor| %.2e  |d critic| %.2e  |d target_actor| %.2e  '
            '|d target_critic| %.2e   bound 5 e = %.2e' % (targets, *worst, bound))
    assert float(fused.actor_optimizer.state[fused.actor.dense1.module.weight]['step']) == 5.0
    assert max(worst) <= bound, (worst, bound)
    assert worst[2] <= worst[0] and worst[3] <= worst[1]
    fused.save_models('standin')
    a2, c2 = ActorNetwork(16, 5), CriticNetwork(21, 1)
    a2.load_state_dict(torch.load(os.path.join(str(tmp_path), 'standin_actor.pt')), strict=True)
    c2.load_state_dict(torch.load(os.path.join(str(tmp_path), 'standin_critic.pt')), strict=True)
    assert all(torch.equal(p.cpu(), q) for p, q in zip(_nets(fused)[3], c2.parameters()))
    fused.load_models('standin')
    assert all(torch.equal(p, q) for p, q in zip(_nets(fused)[3], fused.critic.parameters()))
    fused.batch = _batch(g)
    assert all(bool(torch.isfinite(x)) for x in fused.optimize())      # the optimiser state survives load_models


class _OneBatch(object):
    """What examples/madr_learner.py's Trainer asks of its memory, serving the batch it was last given."""
    batch = None

    def make_index(self, n):
        return None

    def sample_index(self, idx):
        return self.batch


def test_example_learner_switch():
    """examples/madr_learner.py Trainer(fused_optimizer=True) against the same Trainer with the switch off: three optimize() calls,
    same seeds and batches.  With the switch on the learner skips its own clips and soft updates and both happen inside the two
    launches.  Bound on actor and critic: 5 e as in test_accelerate_trainer_optimizer (both sides within their (b) error of float64
    Adam).  The targets: tau of that, plus the two spellings of the Polyak update -- mul_(1 - tau).add_(p, alpha=tau) there,
    t * (1 - tau) + p * tau here -- each at most 1.5 ulp of the result from the exact value, per update."""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'examples'))
    try:
        import madr_learner
    finally:
        sys.path.pop(0)
    from multiagent_rl_amd.critic import CriticNetwork
    from multiagent_rl_amd.optim import FusedAdam
    from multiagent_rl_amd.policy import ActorNetwork
    e = max(_measure('actor', 1.0)['stock'][0], _measure('critic', 1.0)['stock'][0])
    trainers = []
    for switch in (False, True):
        torch.manual_seed(11)
        trainers.append(madr_learner.Trainer(ActorNetwork(16, 5), CriticNetwork(21, 1), _OneBatch(), batch_size=1024, lr=LR,
                                             fused_optimizer=switch))
    plain, fused = trainers
    assert type(plain.actor_optimizer) is torch.optim.Adam and not plain.fused_optimizer
    assert isinstance(fused.actor_optimizer, FusedAdam) and isinstance(fused.critic_optimizer, FusedAdam)
    assert fused.critic_optimizer.max_norm == 0.5 and fused.actor_optimizer.tau == madr_learner.TAU
    start = [t.detach().clone() for t in fused.target_critic.parameters()]
    g = torch.Generator().manual_seed(6)
    for it in range(3):
        plain.memory.batch = fused.memory.batch = _batch(g)
        torch.manual_seed(200 + it)
        lp = plain.optimize()
        torch.manual_seed(200 + it)
        lf = fused.optimize()
        assert all(np.isfinite(x) for x in lp + lf)
    assert fused.critic_optimizer.last_total_norm.is_cuda and float(fused.critic_optimizer.last_total_norm) > 0
    assert all(float(fused.actor_optimizer.state[p]['step']) == 3.0 for p in fused.actor.parameters())
    assert not any(torch.equal(t, s) for t, s in zip(fused.target_critic.parameters(), start))       # the targets moved
    worst = [max(float((a - b).detach().abs().max()) for a, b in zip(x, y)) for x, y in zip(_nets(plain), _nets(fused))]
    t_max = max(float(t.abs().max()) for m in _nets(plain)[2:] for t in m)
    bound_t = madr_learner.TAU * 5.0 * e + 3 * 1.5 * 2.0 ** -23 * t_max
    _report('madr_learner Trainer(fused_optimizer=True) against the switch off, 3 optimize(): |d actor| %.2e  |d critic| %.2e  '
            '|d target_actor| %.2e  |d target_critic| %.2e   bounds 5 e = %.2e, targets %.2e' % (*worst, 5.0 * e, bound_t))
    assert max(worst[:2]) <= 5.0 * e, (worst, e)
    assert max(worst[2:]) <= bound_t, (worst, bound_t)


def test_training_entry_with_the_fused_optimizer(tmp_path, monkeypatch):
    """examples/train_batched.py --critic attention --fused-targets --fused-optimizer on cuda:0 (the pattern of
    tests/test_train_entry.py): the learner it builds has the switch on, every update runs and is finite, the targets it saves
    have moved with the actor and load into plain networks."""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'examples'))
    import madr_learner
    import train_batched as entry
    from multiagent_rl_amd import arglist
    from multiagent_rl_amd.critic import CriticNetwork
    from multiagent_rl_amd.optim import FusedAdam
    losses = []
    inner = madr_learner.Trainer.optimize

    def recording(self):
        assert self.fused_optimizer and isinstance(self.actor_optimizer, FusedAdam) and isinstance(self.critic_optimizer, FusedAdam)
        assert type(self.target_critic).__name__ == '_FusedTarget'
        out = inner(self)
        losses.append(out)
        return out
    monkeypatch.setattr(madr_learner.Trainer, 'optimize', recording)
    saved = (arglist.num_episodes, arglist.save_rate, arglist.warmup_steps, arglist.batch_size)
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        arglist.warmup_steps, arglist.batch_size = 1024, 1024
        res = entry.main(['--scenario', 'simple_spread', '--envs', '256', '--agents', '3', '--episodes', '1024', '--chunk', '50',
                          '--save-rate', '512', '--max-updates-per-chunk', '3', '--out-dir', str(tmp_path / 'Models'),
                          '--critic', 'attention', '--fused-targets', '--fused-optimizer'])
    finally:
        os.chdir(cwd)
        sys.path.pop(0)
        arglist.num_episodes, arglist.save_rate, arglist.warmup_steps, arglist.batch_size = saved
    (name, cnt, st), = res
    assert name == 'simple_spread' and st['updates'] == 6
    assert len(losses) == 6 and np.isfinite(np.array(losses, dtype=np.float64)).all(), losses
    sd = torch.load(tmp_path / 'Models' / 'simple_spread_fin_0_critic.pt')
    CriticNetwork(10 + 5, 1).load_state_dict(sd, strict=True)
    assert all(bool(torch.isfinite(v).all()) for v in sd.values())
