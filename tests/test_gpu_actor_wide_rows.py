"""GPU: the per-step actor at observation rows of 65 .. 104 numbers (simple_spread, local observation, N = 31 .. 50: D = 4 + 2 N).

pw_actor_fused_kernel<S1C> and pw_actor_front_kernel<S1C> at S1C = ceil(D / 8) = 9 .. 13 -- the one-launch actor and the front end of
the three-launch chain.  pw_actor_fused sends every such row to pw_actor_fused_kernel, whatever N is (the 16-wide kernel of N <= 16
keeps rows of at most 64 numbers).

(1) H and the logits within max(2e-5, 2 e32) of the float64 forward (oracle/actor_oracle.py), e32 = the error of stock float32 PyTorch
    (the module itself, on the GPU) against the same float64 forward on the same inputs; the sampled actions equal the host's
    prediction at every (row, head) whose float64 margin exceeds 1e-4.  Random rows x 2 and saturating rows x 30, ragged batches.
(2) The same on the C oracle's simple_spread rows at N = 31, 48, 50.
(3) One launch and chain (PW_ACTOR_NO_FUSE=1): the same bits in H, the logits and the sampled actions.
(4) The loop act = fused(obs); env.step(act) against FusedActor.rollout (pw_policy_rollout3j_kernel, which served these rows before the
    per-step kernels did): the same actions, observations and rewards at every step.
(5) fuse_targets and FusedExploration at N = 31.
(6) What stays refused.

The undecided share of (1) and (2) depends on the float64 logits and the seed alone; every case here was run through
ao.forward_f64 + ao.predict on the host first: no case has an undecided pair (the cap is max(1, pairs / 1000)).

``PW_ACTOR_F64_REPORT=<path>``: measured errors per case are appended there (profiles/actor_vs_f64.txt holds such a run).
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

from oracle import actor_oracle as ao  # noqa: E402  (checker only)
from tests.test_gpu_actor_reference import ATOL, HEADS, VARIANTS, _make_net, _oracle_rows, _report, run_and_compare  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D_OF_S1C = {9: (65, 72), 10: (73, 80), 11: (81, 88), 12: (89, 96), 13: (97, 104)}   # the rows each new instantiation serves
# (D, N): every D at which S1C changes (72 | 73, 80 | 81 stood in for by 81, 88 | 89, 96 | 97), the first and last wide D and N = 48's
# own D = 100 -- odd and even lengths, so that the k < D edge falls in either half-wave; every N of {1, 3, 16, 17, 31, 48, 50, 64, 96}
# occurs -- N <= 16: the routing rule (such rows never go to the 16-wide kernel), N = 96: one environment per workgroup
WIDE_CASES = [(65, 1), (72, 3), (73, 16), (81, 17), (88, 31), (89, 64), (96, 96), (97, 3), (100, 48), (104, 50)]


def _s1c(D):
    return (D + 7) // 8


def _ragged(N, rows=300):
    E = min(16, 96 // N)
    return E * max(1, rows // (E * N)) + 1          # the last workgroup holds one environment


def _net_forward_f32(net, obs):
    """Stock PyTorch float32 on the GPU -> (H [B,N,64], logits [B,N,sum(heads)]) as numpy."""
    import torch.nn.functional as F
    with torch.no_grad():
        x = torch.from_numpy(obs).cuda()
        h = F.relu(net.bilstm(F.relu(net.dense1(x)), None)[0])
        lg = net(x)
        lg = torch.cat(lg, -1) if isinstance(lg, (list, tuple)) else lg
    return h.cpu().numpy(), lg.cpu().numpy()


def _bounds(net, obs, label):
    """-> (atol for H, atol for the logits): max(2e-5, 2 e32), e32 measured here on these very inputs."""
    H64, lg64 = ao.forward_f64(net, obs)
    lg64 = np.concatenate(lg64, -1)
    H32, lg32 = _net_forward_f32(net, obs)
    eH, eL = float(np.abs(H32 - H64).max()), float(np.abs(lg32 - lg64).max())
    _report('%-58s e32: |dH| %.2e  |dlogit| %.2e' % (label + ' stock float32', eH, eL))
    print('%s: stock float32 against float64 |dH| %.3g |dlogit| %.3g' % (label, eH, eL))
    return max(ATOL, 2 * eH), max(ATOL, 2 * eL)


def _compare(fused, net, obs, seed, calls, label, check_act=True):
    aH, aL = _bounds(net, obs, label)
    res = run_and_compare(fused, net, obs, seed, calls, label, atol=aH, check_act=check_act, atol_logit=aL)
    print('%s: |dH| %.3g (bound %.3g) |dlogit| %.3g (bound %.3g) undecided %d / %d' % (label, res['dH'], aH, res['dL'], aL,
                                                                                        res['undecided'], res['pairs']))
    return res


def test_version():
    from multiagent_rl_amd import _lib
    assert _lib.load().pw_version() >= 110


def test_wide_cases_cover_every_new_instantiation():
    assert sorted({_s1c(D) for D, _ in WIDE_CASES}) == [9, 10, 11, 12, 13]
    assert {N for _, N in WIDE_CASES} == {1, 3, 16, 17, 31, 48, 50, 64, 96}
    assert [D for D, _ in WIDE_CASES] == [65, 72, 73, 81, 88, 89, 96, 97, 100, 104]
    for D, _ in WIDE_CASES:
        lo, hi = D_OF_S1C[_s1c(D)]
        assert lo <= D <= hi


@pytest.mark.parametrize('i', range(len(WIDE_CASES)), ids=['D%d-N%d' % c for c in WIDE_CASES])
def test_wide_rows_match_float64(i):
    from multiagent_rl_amd.policy import FusedActor
    D, N = WIDE_CASES[i]
    heads = HEADS[i % len(HEADS)]
    seed, calls, shift = VARIANTS[(i + i // len(VARIANTS)) % len(VARIANTS)]
    net = _make_net(D, heads, shift, seed=N * 100 + D)
    fused = FusedActor(net, seed=seed)
    assert fused.use_fused
    B = _ragged(N)
    rng = np.random.RandomState(N + D)
    label = 'fused<S1C=%d> N=%d D=%d B=%d heads=%s seed=%d call=%d shift=%s' % (_s1c(D), N, D, B, heads, seed, calls, shift)
    _compare(fused, net, (rng.randn(B, N, D) * 2).astype(np.float32), seed, calls, label)
    _compare(fused, net, (rng.randn(B, N, D) * 30).astype(np.float32), seed, calls, label + ' saturated', check_act=False)


@pytest.mark.parametrize('N', [31, 48, 50])
def test_wide_oracle_observation_rows_match_float64(N):
    from multiagent_rl_amd.policy import FusedActor
    obs = _oracle_rows('simple_spread', 9, N)
    D = obs.shape[2]
    assert D == 4 + 2 * N and obs.shape[1] == N
    net = _make_net(D, (5,), 0.0, seed=N)
    fused = FusedActor(net, seed=2 ** 32 + 1)
    _compare(fused, net, obs, fused.seed, 7, 'fused<S1C=%d> simple_spread N=%d D=%d B=%d oracle rows' % (_s1c(D), N, D, obs.shape[0]))


@pytest.mark.parametrize('N,D', [(31, 66), (48, 100), (5, 70), (96, 104)])
def test_one_launch_and_chain_give_the_same_bits(monkeypatch, N, D):
    """Two independent kernels for stage 1 (pw_actor_fused_kernel, pw_actor_front_kernel), two for the recurrence, two for the head.
    The chain's head serves the single 5-logit head only, so the two-head net is compared in H."""
    from multiagent_rl_amd.policy import FusedActor
    B = _ragged(N)
    x = torch.from_numpy((np.random.RandomState(N * D).randn(B, N, D) * 2).astype(np.float32)).cuda()
    for heads in ((5,), (5, 10)):
        net = _make_net(D, heads, 0.0, seed=N + D)
        one = FusedActor(net, seed=2 ** 32 + 5)
        monkeypatch.setenv('PW_ACTOR_NO_FUSE', '1')
        chain = FusedActor(net, seed=2 ** 32 + 5)
        monkeypatch.delenv('PW_ACTOR_NO_FUSE')
        assert one.use_fused and not chain.use_fused and chain.use_mfma_front
        assert torch.equal(one.hidden(x), chain.hidden(x)), (N, D, heads)
        if heads == (5,):
            assert torch.equal(one.logits(x), chain.logits(x))
            one.calls = chain.calls = 2 ** 32 + 3
            assert torch.equal(one(x), chain(x))
            assert one.calls == chain.calls == 2 ** 32 + 4


def test_wide_chain_beyond_96_agents_is_the_default_route():
    from multiagent_rl_amd.policy import FusedActor
    N, D = 100, 65
    net = _make_net(D, (5,), 0.0, seed=3)
    fused = FusedActor(net, seed=2 ** 32 + 9)
    assert fused.use_fused and not fused._one_launch(torch.empty(1, N, D))
    obs = (np.random.RandomState(1).randn(4, N, D) * 2).astype(np.float32)
    _compare(fused, net, obs, fused.seed, 2 ** 32 + 3, 'chain (default route) N=%d D=%d B=4' % (N, D))


@pytest.mark.parametrize('N', [31, 48])
def test_step_loop_equals_the_one_launch_rollout(N):
    """FusedActor.rollout at these N runs pw_policy_rollout3j_kernel, which this test's other side does not touch: the per-step
    kernels reproduce its actions, observations and rewards."""
    from multiagent_rl_amd import make_batched_env
    from multiagent_rl_amd.policy import ActorNetwork, FusedActor
    B, T = 5, 3
    torch.manual_seed(4)
    mk = lambda: make_batched_env('simple_spread', B, n=N, auto_reset=True, max_episode_len=25, seed=21)  # noqa: E731
    env_a, env_b = mk(), mk()
    assert env_a.obs_dim == 4 + 2 * N
    actor = ActorNetwork(env_a.obs_dim, 5).cuda().eval()
    one, loop = FusedActor(actor, seed=9), FusedActor(actor, seed=9)
    obs = env_b.reset()
    assert torch.equal(env_a.reset(), obs)
    got = one.rollout(env_a, T)
    assert env_a.last_kernel().startswith('pw_policy_rollout3j_kernel'), env_a.last_kernel()
    for t in range(T):
        act = loop(obs)
        obs, rew, _, _ = env_b.step(act)
        assert torch.equal(got['act'][t], act), t
        assert torch.equal(got['obs'][t], obs), t
        assert torch.equal(got['rew'][t], rew), t
    assert one.calls == loop.calls == T


def test_learner_plumbing_at_31_agents():
    sys.path.insert(0, os.path.join(ROOT, 'examples'))
    import madr_learner
    from multiagent_rl_amd.critic import CriticNetwork, fuse_targets
    from multiagent_rl_amd.policy import ActorNetwork, FusedActor, FusedExploration
    N, D, b = 31, 66, 33
    torch.manual_seed(7)
    trainer = madr_learner.Trainer(ActorNetwork(D, 5), CriticNetwork(D + 5, 1), None, batch_size=b)
    module = trainer.target_actor
    fa, _ = fuse_targets(trainer)
    assert trainer.target_actor.module is module and fa.use_fused
    s1 = (np.random.RandomState(3).randn(b, N, D) * 2).astype(np.float32)
    _, aL = _bounds(module, s1, 'fuse_targets N=%d D=%d b=%d' % (N, D, b))
    with torch.no_grad():
        want = module(torch.from_numpy(s1).cuda())
    got = trainer.target_actor(torch.from_numpy(s1).cuda())
    assert got.shape == want.shape == (b, N, 5)
    d = float((got - want).abs().max())
    print('fuse_targets N=%d: |target_actor - module| %.3g (bound %.3g)' % (N, d, aL))
    assert d <= aL, (d, aL)

    fx = FusedExploration(trainer.actor, 'Discrete', seed=11)
    ref = FusedActor(trainer.actor, seed=11)
    for call in range(2):
        state = [s1[call, i] for i in range(N)]
        onehot = fx.get_exploration_action(state)
        assert onehot.shape == (1, N, 5) and onehot.dtype == np.float32
        assert np.array_equal(onehot.sum(-1), np.ones((1, N), np.float32)) and set(np.unique(onehot)) == {0.0, 1.0}
        assert ref.calls == call
        idx = ref(torch.from_numpy(s1[call:call + 1]).cuda()).cpu().numpy()
        assert np.array_equal(onehot.argmax(-1), idx)


def test_refusals(monkeypatch):
    from multiagent_rl_amd import _lib
    from multiagent_rl_amd.policy import FusedActor
    lib = _lib.load()
    buf = torch.zeros(1 << 16, dtype=torch.float32, device='cuda')
    out = torch.zeros(1 << 12, dtype=torch.float32, device='cuda')
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    for in_dim in (105, 0):
        rc = lib.pw_actor_fused(p(buf), p(buf), p(buf), p(buf), p(buf), p(buf), p(buf), p(buf), 5, 0, 1, 2, in_dim, 1, 0, 0, None,
                                None, p(out), None, None)
        assert rc == -1 and b'[1, 104]' in lib.pw_last_error(), (in_dim, rc, lib.pw_last_error())
        rc = lib.pw_actor_front(p(buf), p(buf), p(buf), p(buf), 2, in_dim, p(out), None)
        assert rc == -1 and b'[1, 104]' in lib.pw_last_error(), (in_dim, rc, lib.pw_last_error())
    torch.cuda.synchronize()
    net = _make_net(70, (5,), 0.0, seed=1)
    x = torch.zeros(3, 6, 70, device='cuda')
    fused = FusedActor(net, seed=1)
    prev = lib.pw_actor_set_bf16x3(1)
    try:
        with pytest.raises(_lib.PworldError, match='bf16x3.*64'):
            fused.logits(x)
    finally:
        lib.pw_actor_set_bf16x3(prev)
    assert fused.logits(x).shape == (3, 6, 5)
    monkeypatch.setenv('PW_ACTOR_NO_MFMA', '1')
    nomfma = FusedActor(net, seed=1)
    for fn in (nomfma.hidden, nomfma.logits, nomfma):
        with pytest.raises(NotImplementedError, match='PW_ACTOR_NO_MFMA'):
            fn(x)
    assert nomfma.calls == 0
