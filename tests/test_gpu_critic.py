"""GPU: pw_critic_forward (one launch: dense1, LSTM over the agent axis, attention, dense2, optional TD target) and its Python surface.

(a) q against the float64 restatement (tests/critic_ref.py) for the reference's own weights (tests/golden/critic_forward.npz)
    and for freshly initialised ones over N in {1 .. 64}, D in 1 .. 104, A in {5, 15, 16, 1}, b in {1, 15, 16, 17, 600, 1024}:
    ATOL = 2e-5 absolute, the bar of the actor's logits against float64 (tests/test_gpu_actor_reference.py).
(b) A saturating case (inputs x 30 AND LSTM weights x 4).  Its bound is measured in the same run, not assumed:
    e_ref = worst |dq| of stock float32 PyTorch (CriticNetwork on the GPU) against float64 on these inputs; k = on the actor's
    saturated rows, the fused actor's worst |dH| over float32 PyTorch's worst |dH|, both against float64 (what the shared gate
    functions cost relative to float32 PyTorch where the project already accepts them).  The kernel is allowed
    max(2e-5, 2 k e_ref): the factor 2 is for the 64-term dot product in front of the exponential, which the actor does not have.
(c) Index actions and the equal exact one-hots give bit-identical q (one head and two heads).
(d) y == r + gamma * q * (1 - d) formed in torch from the same launch's q, bit for bit.
(e) FusedCritic follows in-place parameter updates; accelerate_trainer(targets=True) on a stand-in Trainer; the training entry
    with the attention critic and fused targets.

``PW_CRITIC_F64_REPORT=<path>``: every case appends its worst |dq| (and float32 PyTorch's own) there
(profiles/critic_vs_f64.txt holds such a run).
"""
import copy
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

from oracle import actor_oracle as ao  # noqa: E402  (checker only)
from tests import critic_ref as cr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ATOL = 2e-5          # tests/test_gpu_actor_reference.py ATOL
GAMMA = 0.95

NS = [1, 2, 3, 6, 7, 12, 16, 17, 24, 31, 48, 64]
DS = [1, 4, 10, 16, 21, 33, 48, 57, 64, 65, 100, 104]
AS = [5, 15, 16, 1]
BS = [1, 15, 16, 17, 600, 1024]
TWO_HEADS = {5: (2, 3), 15: (5, 10), 16: (7, 9)}


def _report(line):
    print(line)
    path = os.environ.get('PW_CRITIC_F64_REPORT')
    if path:
        with open(path, 'a') as f:
            f.write(line + '\n')


def _fresh_cases():
    """(N, D, A, b): every N twice, every D twice (once with a short, once with a long agent axis), every A and b several times."""
    out = []
    for i, N in enumerate(NS):
        out.append((N, DS[i], AS[i % 4], BS[i % 6]))
        out.append((N, DS[(len(NS) - 1 - i + 5) % len(DS)], AS[(i + 2) % 4], BS[(i + 3) % 6]))
    return out


def _net(D, A, seed, lstm_scale=1.0):
    from multiagent_rl_amd.critic import CriticNetwork
    torch.manual_seed(seed)
    net = CriticNetwork(D + A, 1).eval()
    if lstm_scale != 1.0:
        with torch.no_grad():
            for p in net.lstm.parameters():
                p.mul_(lstm_scale)
    return net.cuda()


def _torch_q(net, obs, act):
    with torch.no_grad():
        return net(torch.from_numpy(obs).cuda(), torch.from_numpy(act).cuda())[:, 0].cpu().numpy()


def _measure(net, obs, idx, heads, label):
    """-> (worst |dq| of the kernel, of float32 PyTorch) against float64; asserts the two action forms agree bit for bit."""
    from multiagent_rl_amd.critic import FusedCritic
    fc = FusedCritic(net, heads=heads if len(heads) == 2 else None)
    act = cr.one_hot(idx, heads)
    q64 = cr.forward_f64(net, obs, act)
    x = torch.from_numpy(obs).cuda()
    q_vec = fc.q(x, torch.from_numpy(act).cuda())
    q_idx = fc.q(x, torch.from_numpy(idx if len(heads) == 2 else idx[..., 0]).cuda())
    assert q_vec.shape == (obs.shape[0],) and q_vec.dtype == torch.float32 and not q_vec.requires_grad
    q_vec, q_idx = q_vec.cpu().numpy(), q_idx.cpu().numpy()
    assert np.isfinite(q_vec).all(), label
    assert np.array_equal(q_vec.view(np.uint32), q_idx.view(np.uint32)), '%s: index and one-hot actions differ in %d of %d rows' % (
        label, int((q_vec.view(np.uint32) != q_idx.view(np.uint32)).sum()), q_vec.size)
    dq = float(np.abs(q_vec - q64).max())
    dt = float(np.abs(_torch_q(net, obs, act) - q64).max())
    return dq, dt, float(np.abs(q64).max())


@pytest.mark.parametrize('N,D,heads', cr.GOLDEN_CASES, ids=[cr.golden_name(*c) for c in cr.GOLDEN_CASES])
def test_reference_weights_match_float64(N, D, heads):
    from multiagent_rl_amd.critic import CriticNetwork
    G = np.load(os.path.join(ROOT, 'tests', 'golden', 'critic_forward.npz'))
    name = cr.golden_name(N, D, heads)
    pre = name + '/sd/'
    net = CriticNetwork(D + sum(heads), 1).eval()
    net.load_state_dict({k[len(pre):]: torch.from_numpy(G[k]) for k in G.files if k.startswith(pre)}, strict=True)
    net = net.cuda()
    obs, idx = cr.golden_inputs(N, D, heads)
    dq, dt, qmax = _measure(net, obs, idx, heads, name)
    from multiagent_rl_amd.critic import FusedCritic
    q = FusedCritic(net).q(torch.from_numpy(obs).cuda(), torch.from_numpy(cr.one_hot(idx, heads)).cuda()).cpu().numpy()
    dref = float(np.abs(q - G[name + '/q64'][:, 0]).max())       # against the REFERENCE's own float64 output
    _report('%-52s |dq| %.2e  pytorch-f32 %.2e  |q| <= %.3g  vs reference f64 %.2e' % ('reference ' + name, dq, dt, qmax, dref))
    assert dq <= ATOL and dref <= ATOL, '%s: |dq| %.3g, against the reference %.3g (bound %.3g)' % (name, dq, dref, ATOL)


@pytest.mark.parametrize('N,D,A,b', _fresh_cases(), ids=['N%d-D%d-A%d-b%d' % c for c in _fresh_cases()])
def test_fresh_weights_match_float64(N, D, A, b):
    net = _net(D, A, seed=1000 * N + D)
    rng = np.random.RandomState(N * 131 + D)
    for heads in [(A,)] + ([TWO_HEADS[A]] if A in TWO_HEADS else []):
        obs = (rng.randn(b, N, D) * 2).astype(np.float32)
        idx = np.stack([rng.randint(0, n, (b, N)) for n in heads], -1).astype(np.int32)
        label = 'N=%d D=%d A=%d b=%d heads=%s' % (N, D, A, b, heads)
        dq, dt, qmax = _measure(net, obs, idx, heads, label)
        _report('%-52s |dq| %.2e  pytorch-f32 %.2e  |q| <= %.3g' % (label, dq, dt, qmax))
        assert dq <= ATOL, '%s: |dq| %.3g (bound %.3g)' % (label, dq, ATOL)


def test_float_action_that_is_not_one_hot():
    """What a Trainer passes is the straight-through one-hot (y_hard - y_soft.detach() + y_soft): not always exactly 0 / 1."""
    N, D, A, b = 6, 16, 5, 600
    net = _net(D, A, seed=5)
    rng = np.random.RandomState(3)
    obs = rng.randn(b, N, D).astype(np.float32)
    act = (cr.one_hot(rng.randint(0, A, (b, N, 1)), (A,)) + rng.randn(b, N, A) * 1e-7 + rng.rand(b, N, A) * 0.3).astype(np.float32)
    from multiagent_rl_amd.critic import FusedCritic
    q = FusedCritic(net).q(torch.from_numpy(obs).cuda(), torch.from_numpy(act).cuda()).cpu().numpy()
    dq = float(np.abs(q - cr.forward_f64(net, obs, act)).max())
    _report('%-52s |dq| %.2e' % ('soft action N=6 D=16 A=5 b=600', dq))
    assert dq <= ATOL


@pytest.fixture(scope='module')
def gate_cost():
    """k: on the actor's saturated rows (inputs x 30; tests/test_gpu_actor_reference.py), the fused actor's worst |dH| over
    float32 PyTorch's worst |dH|, both against the float64 forward."""
    import torch.nn.functional as F
    from multiagent_rl_amd.policy import ActorNetwork, FusedActor
    worst_fused = worst_torch = 0.0
    for N, D, seed in ((6, 16, 616), (3, 10, 310), (12, 48, 1248)):
        torch.manual_seed(seed)
        net = ActorNetwork(D, 5).eval().cuda()
        obs = (np.random.RandomState(N + D).randn(601, N, D) * 30).astype(np.float32)
        H64, _ = ao.forward_f64(net, obs)
        x = torch.from_numpy(obs).cuda()
        with torch.no_grad():
            Ht = F.relu(net.bilstm(F.relu(net.dense1(x)), None)[0]).cpu().numpy()
        Hf = FusedActor(net, seed=1).hidden(x).cpu().numpy()
        worst_fused = max(worst_fused, float(np.abs(Hf - H64).max()))
        worst_torch = max(worst_torch, float(np.abs(Ht - H64).max()))
    k = worst_fused / worst_torch
    _report('gate cost on the actor\'s saturated rows: fused |dH| %.2e / pytorch-f32 |dH| %.2e = k %.3g' % (worst_fused, worst_torch, k))
    return k


@pytest.mark.parametrize('N,D,A,b', [(6, 16, 5, 600), (3, 10, 5, 1024), (24, 40, 15, 600), (48, 100, 5, 130)],
                         ids=lambda v: str(v))
def test_saturating_inputs_within_the_measured_bound(gate_cost, N, D, A, b):
    net = _net(D, A, seed=77 + N, lstm_scale=4.0)
    rng = np.random.RandomState(N * 7 + D)
    obs = (rng.randn(b, N, D) * 30).astype(np.float32)
    heads = (A,)
    idx = rng.randint(0, A, (b, N, 1)).astype(np.int32)
    act = cr.one_hot(idx, heads)
    _, steps, score = cr.forward_f64(net, obs, act, want_steps=True)
    label = 'saturating N=%d D=%d A=%d b=%d' % (N, D, A, b)
    dq, e_ref, qmax = _measure(net, obs, idx, heads, label)
    bound = max(ATOL, 2.0 * gate_cost * e_ref)
    _report('%-52s |dq| %.2e  e_ref (pytorch-f32) %.2e  k %.3g  bound %.2e  |q| <= %.3g  |score| <= %.3g  max|h| %.4f' % (
        label, dq, e_ref, gate_cost, bound, qmax, float(np.abs(score).max()), float(np.abs(steps).max())))
    assert float(np.abs(score).max()) > 10.0, 'the case is meant to drive the attention scores to tens'
    assert dq <= bound, '%s: |dq| %.3g exceeds max(2e-5, 2 k e_ref) = %.3g (k %.3g, e_ref %.3g)' % (label, dq, bound, gate_cost, e_ref)


@pytest.mark.parametrize('N,D,heads,b', [(6, 16, (5,), 1024), (2, 21, (5, 10), 17), (48, 100, (5,), 33)], ids=lambda v: str(v))
def test_td_target_is_the_expression_on_the_launchs_own_q(N, D, heads, b):
    from multiagent_rl_amd.critic import FusedCritic
    A = sum(heads)
    net = _net(D, A, seed=N)
    fc = FusedCritic(net, heads=heads if len(heads) == 2 else None)
    g = torch.Generator().manual_seed(N)
    obs = torch.randn(b, N, D, generator=g).cuda()
    idx = torch.stack([torch.randint(0, n, (b, N), generator=g) for n in heads], -1).to(torch.int32).cuda()
    idx = idx if len(heads) == 2 else idx[..., 0]
    r = (torch.randn(b, generator=g) * 3).cuda()
    for d in (torch.zeros(b), torch.ones(b), (torch.rand(b, generator=g) < 0.3).float()):
        d = d.cuda()
        y, q = fc.td_target(obs, idx, r, d, GAMMA, return_q=True)
        want = r + GAMMA * q * (1. - d)              # ddpg_gumbel_fix.py:154 on this launch's q
        assert y.shape == (b,) and not y.requires_grad
        assert torch.equal(y.view(torch.int32), want.view(torch.int32)), (N, int((y != want).sum()))
        assert torch.equal(q, fc.q(obs, idx))       # the epilogue does not change q
    assert torch.equal(fc.td_target(obs, idx, r, d, GAMMA), y)


def test_every_instantiation_opts_in_to_its_own_lds():
    """The host side launches all three forms through one launcher template; the opt-in to more than 64 KiB of LDS is remembered per
    kernel.  N = 32 needs 146.5 KiB, so in ONE process every instantiation of the attention form (KO in {4, 8, 16, 26} x KA in {2, 4})
    and then every one of the model form is launched at b = 17 (a full workgroup and one row): a kernel whose opt-in another
    kernel's had masked would fail its launch.  q (and r_pred) against float64 as everywhere in this file."""
    from multiagent_rl_amd.critic import CriticNetwork, FusedCritic, ModelCriticNetwork
    from tests import model_ref as mr
    N, b = 32, 17
    rng = np.random.RandomState(32)
    for cls in (CriticNetwork, ModelCriticNetwork):
        for D in (4, 20, 40, 100):
            for A in (5, 15):
                torch.manual_seed(D + A)
                net = cls(D + A, 1).eval().cuda()
                obs = (rng.randn(b, N, D) * 2).astype(np.float32)
                idx = rng.randint(0, A, (b, N, 1)).astype(np.int32)
                act = cr.one_hot(idx, (A,))
                got = FusedCritic(net)(torch.from_numpy(obs).cuda(), torch.from_numpy(idx[..., 0]).cuda())
                if cls is ModelCriticNetwork:
                    assert got[0].shape == (b, 1) and got[1].shape == (b, 1)
                    got, want = np.stack([g[:, 0].cpu().numpy() for g in got]), np.stack(mr.critic_f64(net, obs, act))
                else:
                    assert got.shape == (b, 1)
                    got, want = got[:, 0].cpu().numpy(), cr.forward_f64(net, obs, act)
                worst = float(np.abs(got - want).max())
                _report('%-52s |d| %.2e' % ('%s N=32 D=%d A=%d b=17' % (cls.__name__, D, A), worst))
                assert worst <= ATOL, (cls.__name__, D, A, worst)


def _soft_update(target, source, tau):
    for tp, sp in zip(target.parameters(), source.parameters()):        # ddpg_gumbel_fix.py:37-48
        tp.data.copy_(tp.data * (1.0 - tau) + sp.data * tau)


def test_fused_critic_follows_in_place_updates_and_returns_b_by_1():
    from multiagent_rl_amd.critic import FusedCritic
    N, D, A, b = 6, 16, 5, 300
    target, source = _net(D, A, seed=1), _net(D, A, seed=2)
    fc = FusedCritic(target)
    rng = np.random.RandomState(0)
    obs = (rng.randn(b, N, D) * 2).astype(np.float32)
    act = cr.one_hot(rng.randint(0, A, (b, N, 1)), (A,))
    x, a = torch.from_numpy(obs).cuda(), torch.from_numpy(act).cuda()
    before = fc(x, a)
    assert before.shape == (b, 1) and not before.requires_grad
    assert torch.equal(fc.forward(x, [a[..., :2], a[..., 2:]]), before)          # a list is concatenated as the module does
    assert float(np.abs(before[:, 0].cpu().numpy() - cr.forward_f64(target, obs, act)).max()) <= ATOL
    _soft_update(target, source, 0.5)
    after = fc(x, a)[:, 0].cpu().numpy()
    q64 = cr.forward_f64(target, obs, act)
    assert float(np.abs(after - q64).max()) <= ATOL
    assert float(np.abs(after - before[:, 0].cpu().numpy()).max()) > 100 * ATOL     # the update is large: the old weights would miss
    with pytest.raises(RuntimeError):
        FusedCritic(copy.deepcopy(target).cpu())


class _StandInTrainer(object):
    """The surface of the reference's Trainer that accelerate_trainer touches, written for this test: target nets as deep copies,
    soft_update / hard_update over parameters(), an optimize() that evaluates the three no-gradient lines of
    ddpg_gumbel_fix.py:148-154 (and moves the online nets, so that the soft update has something to carry), save / load
    through state_dict()."""

    def __init__(self, actor, critic, out_dir):
        self.device = torch.device('cuda', torch.cuda.current_device())
        self.actor, self.critic = actor.to(self.device), critic.to(self.device)
        self.target_actor, self.target_critic = copy.deepcopy(self.actor), copy.deepcopy(self.critic)
        self.target_actor.eval()
        self.target_critic.eval()
        self.action_type, self.out_dir, self.batch, self.last = 'Discrete', out_dir, None, None

    def soft_update(self, target, source, tau):
        _soft_update(target, source, tau)

    def hard_update(self, target, source):
        for tp, sp in zip(target.parameters(), source.parameters()):
            tp.data.copy_(sp.data)

    def gumbel_softmax(self, x):
        n, t = x.size(0), x.size(1)
        y = torch.nn.functional.gumbel_softmax(x.contiguous().view(n * t, x.size(2)), hard=True)
        return y.contiguous().view(n, t, -1)

    def optimize(self):
        s1, r, d = self.batch
        logits1 = self.target_actor.forward(s1)
        a1 = self.gumbel_softmax(logits1)
        q_next = self.target_critic.forward(s1, a1)
        q_next = torch.squeeze(q_next.detach())
        y_expected = r + GAMMA * q_next * (1. - d)
        self.last = dict(logits1=logits1.detach().clone(), a1=a1.detach().clone(), y=y_expected.clone())
        with torch.no_grad():
            for net in (self.actor, self.critic):
                for p in net.parameters():
                    p.add_(0.05 * torch.sign(p))
        self.soft_update(self.target_actor, self.actor, 0.5)
        self.soft_update(self.target_critic, self.critic, 0.5)
        return y_expected

    def save_models(self, fname):
        torch.save(self.target_actor.state_dict(), os.path.join(self.out_dir, fname + '_actor.pt'))
        torch.save(self.target_critic.state_dict(), os.path.join(self.out_dir, fname + '_critic.pt'))

    def load_models(self, fname):
        self.actor.load_state_dict(torch.load(os.path.join(self.out_dir, fname + '_actor.pt')))
        self.critic.load_state_dict(torch.load(os.path.join(self.out_dir, fname + '_critic.pt')))
        self.hard_update(self.target_actor, self.actor)
        self.hard_update(self.target_critic, self.critic)


def _trainer(tmp_path):
    from multiagent_rl_amd.critic import CriticNetwork
    from multiagent_rl_amd.policy import ActorNetwork
    torch.manual_seed(11)
    return _StandInTrainer(ActorNetwork(16, 5), CriticNetwork(21, 1), str(tmp_path))


def test_accelerate_trainer_targets(tmp_path):
    from multiagent_rl_amd.critic import CriticNetwork, accelerate_trainer
    from multiagent_rl_amd.policy import ActorNetwork
    N, D, b = 6, 16, 1024
    plain, fused = _trainer(tmp_path), _trainer(tmp_path)
    ta, tc = plain.target_actor, plain.target_critic
    accelerate_trainer(plain, seed=3)                                    # targets=False: both attributes the very same objects
    assert plain.target_actor is ta and plain.target_critic is tc
    fa_mod, fc_mod = fused.target_actor, fused.target_critic
    accelerate_trainer(fused, seed=3, targets=True)
    assert fused.target_actor is not fa_mod and fused.target_actor.module is fa_mod and fused.target_critic.module is fc_mod
    assert [p.data_ptr() for p in fused.target_critic.parameters()] == [p.data_ptr() for p in fc_mod.parameters()]
    assert sorted(fused.target_critic.state_dict()) == sorted(fc_mod.state_dict())
    assert fused.target_actor.eval() is fa_mod and fused.target_critic.train() is fc_mod and fused.target_critic.eval() is fc_mod
    g = torch.Generator().manual_seed(5)
    for it in range(3):                      # the second and third round run on soft-updated targets
        batch = ((torch.randn(b, N, D, generator=g) * 2).cuda(), (torch.randn(b, generator=g) * 3).cuda(),
                 (torch.rand(b, generator=g) < 0.2).float().cuda())
        plain.batch = fused.batch = batch
        torch.manual_seed(100 + it)
        plain.optimize()
        torch.manual_seed(100 + it)
        y = fused.optimize()
        assert y.shape == (b,) and not y.requires_grad
        dl = float((plain.last['logits1'] - fused.last['logits1']).abs().max())
        assert dl <= ATOL, (it, dl)
        same = (plain.last['a1'].argmax(-1) == fused.last['a1'].argmax(-1)).all(dim=1)     # rows whose sampled a1 agree
        assert float(same.float().mean()) > 0.99, (it, float(same.float().mean()))
        dy = float((plain.last['y'] - fused.last['y'])[same].abs().max())
        _report('accelerate_trainer(targets=True) round %d: |dlogits1| %.2e  |dy| %.2e on %d of %d rows with the same a1' % (
            it, dl, dy, int(same.sum()), b))
        assert dy <= ATOL, (it, dy)
        # soft updates reached the wrapped modules: both trainers' targets hold the same numbers
        for pp, pf in zip(list(plain.target_actor.parameters()) + list(plain.target_critic.parameters()),
                          list(fa_mod.parameters()) + list(fc_mod.parameters())):
            assert torch.equal(pp, pf)
    fused.save_models('standin')
    a2, c2 = ActorNetwork(16, 5), CriticNetwork(21, 1)
    a2.load_state_dict(torch.load(os.path.join(str(tmp_path), 'standin_actor.pt')), strict=True)   # plain modules load the files
    c2.load_state_dict(torch.load(os.path.join(str(tmp_path), 'standin_critic.pt')), strict=True)
    assert all(torch.equal(p.cpu(), q) for p, q in zip(fc_mod.parameters(), c2.parameters()))
    fused.load_models('standin')             # hard updates through the wrappers; the actor snapshots are refreshed behind it
    assert all(torch.equal(p, q) for p, q in zip(fc_mod.parameters(), fused.critic.parameters()))
    x = batch[0]
    with torch.no_grad():
        want = fa_mod(x)
    assert float((fused.target_actor.forward(x) - want).abs().max()) <= ATOL
    assert float((fused.target_actor(x) - want).abs().max()) <= ATOL


def test_training_entry_with_the_attention_critic_and_fused_targets(tmp_path, monkeypatch):
    """examples/train_batched.py --critic attention --fused-targets on cuda:0 (the pattern of tests/test_train_entry.py): finishes,
    the updates are counted, every loss is finite, and the saved critic loads into a plain CriticNetwork."""
    sys.path.insert(0, os.path.join(ROOT, 'examples'))
    import madr_learner
    import train_batched as entry
    from multiagent_rl_amd import arglist
    from multiagent_rl_amd.critic import CriticNetwork
    losses = []
    inner = madr_learner.Trainer.optimize

    def recording(self):
        assert type(self.target_critic).__name__ == '_FusedTarget' and type(self.target_actor).__name__ == '_FusedTarget'
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
                          '--critic', 'attention', '--fused-targets'])
    finally:
        os.chdir(cwd)
        arglist.num_episodes, arglist.save_rate, arglist.warmup_steps, arglist.batch_size = saved
    (name, cnt, st), = res
    assert name == 'simple_spread' and st['episodes'] == 1024 and st['env_steps'] == 100 * 256 and st['updates'] == 6
    assert len(losses) == 6 and np.isfinite(np.array(losses, dtype=np.float64)).all(), losses
    sd = torch.load(tmp_path / 'Models' / 'simple_spread_fin_0_critic.pt')
    CriticNetwork(10 + 5, 1).load_state_dict(sd, strict=True)
