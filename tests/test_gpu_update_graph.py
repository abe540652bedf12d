"""GPU: the learner's update as one captured graph (multiagent_rl_amd/graph.py) and the three device-side pieces it rests on.

* pw_replay_sample: the drawn slots equal the Python restatement of the rule (tests/test_update_graph_host.py), every gathered tensor
  equals pw_replay_gather on those slots bit for bit (row, two-head, per-agent and STATE rings), the length cell bounds the draw
  whatever it holds, and a captured draw follows the ring as it grows.
* pw_adam_step_dev against pw_adam_step: bit-identical parameters, moments, targets and norm at every one of 25 steps, eagerly and as
  25 replays of one captured step.
* FusedActor.refresh(in_place=True): every buffer keeps its address and holds what a fresh FusedActor holds.
* The update itself.  Three example learners start from one deep copy: A and B eager, C graphed.  A against B shows that the eager
  update is reproducible bit for bit on this stack (it is: every kernel of this package sums in a fixed order, and the rocBLAS GEMMs and
  elementwise ops of the stock part gave equal bits in every run measured); C against A must then be bit-identical after EVERY update --
  the soft update moves the targets each step, so a stale target actor, a frozen Adam step or a frozen ring length each breaks it.
"""
import copy
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from multiagent_rl_amd import _lib
from tests.test_update_graph_host import draw_restated

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'examples'))

CAP, FILLED, SEED = 256, 100, 12345678


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _same(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                                              b.view(torch.int32) if b.dtype == torch.float32 else b)


# ---- rings of recognisable content -----------------------------------------------------------------------------------------------
def _ring(kind, filled=FILLED, seed=SEED):
    """capacity 256, `filled` transitions written straight into the planes: every number is a function of its slot and position."""
    from multiagent_rl_amd.replay_buffer import ReplayBuffer
    kw, N, D = {}, 3, 10
    if kind == 'two_head':
        kw, N, D = dict(act_heads=(5, 10)), 2, 21
    elif kind == 'per_agent':
        kw = dict(per_agent=True)
    elif kind == 'state_spread':
        kw = dict(state_ring=dict(scenario='simple_spread', num_landmarks=3, num_adversaries=0))
    elif kind == 'state_tag':
        kw, N, D = dict(state_ring=dict(scenario='simple_tag', num_landmarks=2, num_adversaries=3)), 4, 16
    rb = ReplayBuffer(CAP, N, D, device_index='counter', index_seed=seed, **kw)
    g = torch.Generator().manual_seed(5)
    for name in ('obs', 'next_obs', 'rew', 'done') + (('lm',) if rb.lm is not None else ()):
        plane = getattr(rb, name)
        slot = torch.arange(CAP, dtype=torch.float32).view(-1, *([1] * (plane.dim() - 1)))
        plane.copy_((torch.rand(plane.shape, generator=g) + slot).cuda())       # integer part = the slot
    heads = rb.act_heads
    act = torch.stack([torch.randint(0, h, (CAP, N), generator=g) for h in heads], -1).to(torch.uint8)
    rb.act.copy_((act if len(heads) == 2 else act[..., 0]).cuda())
    rb._next_idx, rb._len = filled % CAP, filled
    return rb


RINGS = ['row', 'two_head', 'per_agent', 'state_spread', 'state_tag']


@pytest.mark.parametrize('b', [1, 5, 64, 257])
@pytest.mark.parametrize('kind', RINGS)
def test_sample_draws_by_the_rule_and_gathers_like_pw_replay_gather(kind, b):
    rb = _ring(kind)
    lib = rb._lib
    first = rb.make_index(b)                                              # the draw alone: draw number 0
    want = draw_restated(SEED, 0, b, FILLED)
    assert first.dtype == torch.int64 and np.array_equal(first.cpu().numpy(), want)
    assert int(rb._cells[0]) == 1 and int(rb._cells[1]) == FILLED
    ref = rb.sample_index(first)                                          # pw_replay_gather on those slots
    rb.reset_draws(0)
    got = rb.sample(b)                                                    # draw and gather, one launch
    assert all(_same(x, y) for x, y in zip(got, ref)), kind
    assert 0 <= float(got[2].floor().min()) and float(got[2].floor().max()) < FILLED      # rew = slot + a fraction
    # the one-launch form with out_idx, and only some of the outputs
    idx = torch.full((b,), -1, dtype=torch.int64, device='cuda')
    rew = torch.empty_like(ref[2])
    nxt = torch.empty_like(ref[3])
    rb.reset_draws(0)
    _lib.check(lib.pw_replay_sample(C.byref(rb._store), SEED, _p(rb._cells), _p(rb._cells[1:]), b, _p(idx), None, None, _p(rew), _p(nxt), None,
                                    rb._stream()))
    assert torch.equal(idx, first) and _same(rew, ref[2]) and _same(nxt, ref[3])
    assert int(rb._cells[0]) == 0                                          # the launch itself does not advance the counter
    # the next draw differs, and the sequence repeats from a reset counter
    rb.reset_draws(1)
    second = rb.make_index(b)
    assert np.array_equal(second.cpu().numpy(), draw_restated(SEED, 1, b, FILLED))
    if b >= 5:
        assert not torch.equal(first, second)
    rb.reset_draws(0)
    assert torch.equal(rb.make_index(b), first) and torch.equal(rb.make_index(b), second)


@pytest.mark.parametrize('kind', ['row', 'state_tag'])
def test_the_length_cell_cannot_send_a_draw_outside_the_ring(kind):
    rb = _ring(kind)
    rb._cells[1:].fill_(0)                       # counts as 1
    assert not rb.make_index(257).any()
    obs = rb.sample(64)[0]
    assert _same(obs, rb.sample_index(torch.zeros(64, dtype=torch.int64, device='cuda'))[0])
    rb._cells[1:].fill_(10 ** 9)                 # counts as the capacity
    rb.reset_draws(3)
    idx = rb.make_index(257)
    assert int(idx.min()) >= 0 and int(idx.max()) < CAP and np.array_equal(idx.cpu().numpy(), draw_restated(SEED, 3, 257, CAP))
    rb._cells[1:].fill_(-(2 ** 40))
    assert not rb.make_index(5).any()
    rb.clear()
    with pytest.raises(ValueError, match='empty'):
        rb.sample(4)


def test_a_captured_draw_follows_the_ring_as_it_grows():
    rb = _ring('row', filled=64)
    rb.make_index(8)                             # warm: nothing is allocated lazily inside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        idx = rb.make_index(256)
    call = int(rb._cells[0])                     # capture ran nothing: the first replay is this draw
    assert call == 1
    g.replay()
    torch.cuda.synchronize()
    assert int(idx.max()) < 64 and np.array_equal(idx.cpu().numpy(), draw_restated(SEED, call, 256, 64))
    B = 64
    rb.add_batch(torch.rand(B, 3, 10), torch.randint(0, 5, (B, 3)), torch.rand(B), torch.rand(B, 3, 10))
    assert len(rb) == 128 and int(rb._cells[1]) == 128
    g.replay()
    torch.cuda.synchronize()
    got = idx.cpu().numpy()
    assert got.min() >= 0 and got.max() < 128 and (got >= 64).any()
    assert np.array_equal(got, draw_restated(SEED, call + 1, 256, 128))
    assert int(rb._cells[0]) == call + 2


# ---- Adam with the step on the device --------------------------------------------------------------------------------------------
LR, BETAS, MAX_NORM, TAU = 1e-2, (0.9, 0.999), 0.5, 1e-2


def _adam_sets(name):
    from tests.test_gpu_optim import _offset_view, _param_set
    params = _param_set(name)
    odd = _offset_view((torch.randn(33, generator=torch.Generator().manual_seed(2)) * 0.1).cuda(), 1).requires_grad_()   # 4-byte offset
    if len(params) < 32:
        params.append(odd)
    else:
        params[-1] = odd
    targets = [t.detach().clone() + 0.5 for t in params]
    return params, targets


def _adam_state(opt, params, targets):
    out = [p.detach().clone() for p in params] + [t.clone() for t in targets] + [opt.last_total_norm.clone()]
    return out + [opt.state[p][k].clone() for p in params for k in ('exp_avg', 'exp_avg_sq')]


@pytest.mark.parametrize('graphed', [False, True], ids=['eager', 'graph'])
@pytest.mark.parametrize('name', ['synthetic', 'exact32'])
def test_adam_step_dev_equals_adam_step_bit_for_bit(name, graphed):
    from multiagent_rl_amd.optim import FusedAdam
    from tests.test_gpu_optim import _grads
    steps = 26 if graphed else 25
    (pa, ta), (pb, tb) = _adam_sets(name), _adam_sets(name)
    host = FusedAdam(pa, lr=LR, betas=BETAS, max_norm=MAX_NORM, targets=ta, tau=TAU)
    dev = FusedAdam(pb, lr=LR, betas=BETAS, max_norm=MAX_NORM, targets=tb, tau=TAU, graph_steps=True)
    rng = np.random.RandomState(8)
    static = [torch.zeros_like(p) for p in pb]
    graph = None
    for it in range(steps):
        gs = _grads(pa, rng, 1.0)
        for p, g in zip(pa, gs):
            p.grad = g
        host.step()
        for p, s, g in zip(pb, static, gs):
            s.copy_(g)
            p.grad = s
        if not graphed or it == 0:
            dev.step()                           # graph: one eager step creates the state and the step cell
        else:
            if graph is None:
                torch.cuda.synchronize()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    dev.step()
            else:
                dev.note_graph_steps(1)
            graph.replay()
        for x, y in zip(_adam_state(host, pa, ta), _adam_state(dev, pb, tb)):
            assert _same(x, y), (name, it)
    assert all(float(dev.state[p]['step']) == steps for p in pb) and int(dev._step_cells[0]) == steps + 1
    ref = torch.optim.Adam(pb, lr=LR, betas=BETAS)
    ref.load_state_dict(dev.state_dict())


def test_a_step_cell_is_not_created_inside_a_capture(monkeypatch):
    """A cell filled inside the captured region would be reset by every replay: the first step() has to be an eager one."""
    from multiagent_rl_amd.optim import FusedAdam
    p = torch.randn(7, device='cuda').requires_grad_()
    p.grad = torch.randn(7, device='cuda')
    opt = FusedAdam([p], graph_steps=True)
    monkeypatch.setattr(torch.cuda, 'is_current_stream_capturing', lambda: True)
    with pytest.raises(RuntimeError, match='eagerly'):
        opt.step()


# ---- the target actor's snapshot in place ----------------------------------------------------------------------------------------
NAMES = ('w1', 'b1', 'wih', 'wih_t', 'bih', 'whh_f', 'whh_r', 'w2', 'b2', 'frag')


@pytest.mark.parametrize('out_dim', [5, [5, 10]], ids=['one_head', 'two_heads'])
def test_refresh_in_place_keeps_every_address_and_equals_a_fresh_snapshot(out_dim):
    from multiagent_rl_amd.policy import ActorNetwork, FusedActor
    torch.manual_seed(4)
    actor = ActorNetwork(21, out_dim).cuda()
    fa = FusedActor(actor)
    where = {k: getattr(fa, k).data_ptr() for k in NAMES}
    with torch.no_grad():
        for p in actor.parameters():
            p.add_(torch.randn_like(p) * 0.05)
    fa.refresh(in_place=True)
    fresh = FusedActor(actor)
    for k in NAMES:
        assert getattr(fa, k).data_ptr() == where[k], k
        assert _same(getattr(fa, k), getattr(fresh, k)), k
    obs = torch.randn(9, 3, 21, device='cuda')
    assert _same(torch.cat(fa.logits(obs), -1) if isinstance(out_dim, list) else fa.logits(obs),
                 torch.cat(fresh.logits(obs), -1) if isinstance(out_dim, list) else fresh.logits(obs))
    fa.actor = ActorNetwork(16, out_dim).cuda()
    with pytest.raises(ValueError, match='shapes are fixed'):
        fa.refresh(in_place=True)


# ---- the update itself -----------------------------------------------------------------------------------------------------------
def _straight_through(logits):
    """The noise-free hard sample: one_hot(argmax) + softmax - softmax.detach() (the gradient of the soft sample, no RNG)."""
    def one(x):
        sm = F.softmax(x, dim=-1)
        return F.one_hot(x.argmax(-1), x.shape[-1]).to(x.dtype) + sm - sm.detach()
    return torch.cat([one(x) for x in logits], -1) if isinstance(logits, (list, tuple)) else one(logits)


VARIANTS = {   # name -> (Trainer class, actor factory, critic factory, ring kwargs, N, D)
    'attention': ('Trainer', lambda pol, cr: pol.ActorNetwork(10, 5), lambda pol, cr: cr.CriticNetwork(15, 1), {}, 3, 10),
    'two_head': ('Trainer', lambda pol, cr: pol.ActorNetwork(21, [5, 10]), lambda pol, cr: cr.CriticNetwork(36, 1), dict(act_heads=(5, 10)), 2, 21),
    'bicnet': ('BiCNetTrainer', lambda pol, cr: pol.ActorNetwork(10, 5), lambda pol, cr: cr.BiCNetCritic(15, 1), dict(per_agent=True), 3, 10),
    'model': ('ModelTrainer', lambda pol, cr: pol.ModelActorNetwork(10, 5), lambda pol, cr: cr.ModelCriticNetwork(15, 1), {}, 3, 10),
}
BATCH = 33


def _filled_memory(ring_kw, N, D, n=200):
    from multiagent_rl_amd.replay_buffer import ReplayBuffer
    rb = ReplayBuffer(256, N, D, device_index='counter', index_seed=77, **ring_kw)
    g = torch.Generator().manual_seed(9)
    heads = ring_kw.get('act_heads', (5,))
    act = torch.stack([torch.randint(0, h, (n, N), generator=g) for h in heads], -1)
    rew = torch.randn((n, N) if ring_kw.get('per_agent') else (n,), generator=g)
    rb.add_batch(torch.randn(n, N, D, generator=g), act if len(heads) == 2 else act[..., 0], rew, torch.randn(n, N, D, generator=g),
                 done=(torch.rand(rew.shape, generator=g) < 0.1).float())
    return rb


def _learner(variant, nets, graph, noise_free=True):
    import madr_learner
    from multiagent_rl_amd.policy import accelerate_trainer
    cls_name, _, _, ring_kw, N, D = VARIANTS[variant]
    base = getattr(madr_learner, cls_name)
    cls = type('NoiseFree' + cls_name, (base,), {'_sample': staticmethod(_straight_through)}) if noise_free else base
    actor, critic = copy.deepcopy(nets)
    torch.manual_seed(21)
    t = cls(actor, critic, _filled_memory(ring_kw, N, D), action_type='MultiDiscrete' if 'act_heads' in ring_kw else 'Discrete', batch_size=BATCH, fused_optimizer=True, fused_lstm=True, fused_attention=True,
            graph_update=graph)
    if not graph:
        accelerate_trainer(t, targets=True)
    return t


def _everything(t):
    out = []
    for net in (t.actor, t.critic, t.target_actor, t.target_critic):
        out += [p.detach().clone() for p in net.parameters()]
    for opt in (t.actor_optimizer, t.critic_optimizer):
        for group in opt.param_groups:
            for p in group['params']:
                st = opt.state.get(p)
                if st:
                    out += [st['exp_avg'].clone(), st['exp_avg_sq'].clone()]
    return out


@pytest.mark.parametrize('variant', list(VARIANTS))
def test_graphed_updates_equal_eager_updates_bit_for_bit(variant):
    from multiagent_rl_amd import critic as cr, policy as pol
    from multiagent_rl_amd.graph import GraphedUpdate
    torch.manual_seed(3)
    nets = (VARIANTS[variant][1](pol, cr), VARIANTS[variant][2](pol, cr))
    a, b, c = _learner(variant, nets, False), _learner(variant, nets, False), _learner(variant, nets, True)
    assert isinstance(c.optimize, GraphedUpdate) and not isinstance(a.optimize, GraphedUpdate)
    for it in range(8):
        la, lb = a.optimize(), b.optimize()
        lc = tuple(float(x) for x in c.optimize())
        sa, sb, sc = _everything(a), _everything(b), _everything(c)
        assert len(sa) == len(sc) > 20
        worst_ab = max(float((x - y).abs().max()) for x, y in zip(sa, sb))
        print('%s update %d: losses A %r C %r, max |A - B| %.3e' % (variant, it + 1, la, lc, worst_ab))
        # A against B: the eager update is reproducible bit for bit (no stock op in it was seen to differ between two runs) ...
        assert la == lb and all(_same(x, y) for x, y in zip(sa, sb)), (variant, it, worst_ab)
        # ... so the graphed update is held to the same: bit-identical to the eager one after every update
        bad = [i for i, (x, y) in enumerate(zip(sa, sc)) if not _same(x, y)]
        assert not bad and la == lc, (variant, it, bad[:5], la, lc)
    g = c.optimize
    assert (g.eager_calls, g.captures, g.replays) == (3, 1, 5) and c.iter == a.iter == 8
    assert g.losses() == lc
    for opt in (c.actor_optimizer, c.critic_optimizer):
        assert all(float(opt.state[p]['step']) == 8.0 for grp in opt.param_groups for p in grp['params'])
        assert int(opt._step_cells[0]) == 9
        ref = torch.optim.Adam([p for grp in opt.param_groups for p in grp['params']], lr=1e-2)
        ref.load_state_dict(opt.state_dict())
        assert all(float(st['step']) == 8.0 for st in ref.state.values())
    # a changed learning rate travels as a kernel argument: the update is captured again, and keeps following the eager learner
    for t in (a, c):
        for opt in (t.actor_optimizer, t.critic_optimizer):
            opt.param_groups[0]['lr'] = 1e-3
    la, lc = a.optimize(), tuple(float(x) for x in c.optimize())
    assert g.captures == 2 and la == lc and all(_same(x, y) for x, y in zip(_everything(a), _everything(c)))


def test_graphed_updates_with_real_gumbel_sampling():
    from multiagent_rl_amd import critic as cr, policy as pol
    torch.manual_seed(3)
    t = _learner('attention', (pol.ActorNetwork(10, 5), cr.CriticNetwork(15, 1)), True, noise_free=False)
    nets = lambda: [p.detach().clone() for net in (t.actor, t.critic, t.target_actor, t.target_critic) for p in net.parameters()]  # noqa: E731
    losses, before = [], nets()
    for it in range(12):
        losses.append(tuple(float(x) for x in t.optimize()))
        after = nets()
        assert all(bool(torch.isfinite(x).all()) for x in _everything(t))
        # Adam moves every tensor that has a gradient by about lr, the soft update every target with it: none stays as it was
        same = [i for i, (x, y) in enumerate(zip(before, after)) if _same(x, y)]
        assert not same, (it, same)
        before = after
    assert np.isfinite(np.array(losses)).all()
    replayed = losses[3:]
    assert len(set(replayed)) > 1, replayed                                 # a replay that repeated its batch and noise would repeat its losses


def test_train_batched_with_the_graphed_update(tmp_path, monkeypatch):
    import madr_learner
    from multiagent_rl_amd import make_batched_env
    from multiagent_rl_amd.critic import CriticNetwork
    from multiagent_rl_amd.policy import ActorNetwork
    from multiagent_rl_amd.train import train_batched

    class Args(object):
        max_episode_len, num_episodes, is_training = 25, 48, True
        batch_size, warmup_steps, update_rate, save_rate, display = 32, 100, 40, 16, False

    made = []

    def Trainer(actor, critic, memory, action_type='Discrete'):
        made.append(madr_learner.Trainer(actor, critic, memory, action_type=action_type, batch_size=32, fused_optimizer=True, fused_lstm=True,
                                         fused_attention=True, graph_update=True))
        return made[-1]
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(1)
    env = make_batched_env('simple_spread', 16, auto_reset=True, max_episode_len=25, seed=5, n=3)
    hist = train_batched(env, ActorNetwork(env.obs_dim, 5), CriticNetwork(env.obs_dim + 5, 1), Trainer, 'simple_spread', 'Discrete',
                         arglist=Args(), out_dir=str(tmp_path), log=lambda *a: None, chunk=25, max_updates_per_chunk=4, graph_update=True)
    st = hist['stats']
    learner, = made
    assert learner.memory.device_index == 'counter' and len(learner.memory) == st['env_steps']
    assert st['updates_run'] > 3 and st['graph_replays'] == st['updates_run'] - 3 > 0, st
    assert all(bool(torch.isfinite(p).all()) for net in (learner.actor, learner.critic, learner.target_actor) for p in net.parameters())
    assert {'reward_episodes', 'reward_episodes_by_agents', 'open_episodes', 'stats'} <= set(hist)
    assert all(float(learner.actor_optimizer.state[p]['step']) == st['updates_run'] for p in learner.actor.parameters())
