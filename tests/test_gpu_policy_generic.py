"""GPU: the generic one-launch policy rollout (pw_policy_rollout_generic_kernel: actor + Gumbel sampling + pw_rollout_kernel's
environment step for a whole chunk in ONE kernel) -- every simple_spread / simple_tag configuration the specialised rollout forms
refuse: the full observation (make_env(local_observation=False), experiments/scenarios.py:124), L > N, per-agent sizes /
accelerations / speed clamps, a simple_tag roster with one agent unlike its role, dispatch=dict(force_generic=1).

Method of tests/test_gpu_policy_oracle.py: the env and the float32 C oracle are built from the same configuration and the same Philox
reset; the actions a launch sampled (an output) are replayed through the oracle, and every environment output of the launch -- obs,
rew, rew_shared, terminal, done, final_obs at terminal steps, the final pos / vel / landmarks / ep_step / ep_count -- equals the
oracle's BIT FOR BIT.  So that a run without a single contact cannot pass as parity, the oracle's own collision masks over the replay
must show an agent-agent contact in at least 10 env-steps (cases 1 - 7).  Then HIP against HIP: the generic form against the
specialised forms on handles both serve, against the per-step FusedActor + env.step loop, the ring sink against BatchedRollout.collect,
the sink's refusals, and train_batched end to end on a full-observation env.
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

from oracle import c_oracle as co  # noqa: E402  (checker only)
from tests.test_gpu_actor_reference import assert_rollout_actions_match_f64  # noqa: E402
from tests.test_gpu_parity import _assert_same_bits, _np  # noqa: E402
from tests.test_gpu_policy_oracle import _assert_final_state, _replay_through_oracle  # noqa: E402
from tests.test_gpu_world_constants import _mk  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GENERIC = 'pw_policy_rollout_generic_kernel'
AUTO = dict(force_generic=0, no_stream=0, duo=-1, quad=-1, obs_block=-1, trio=-1, p_prio=-1, envs_per_wave=0, policy_form=0)
MIN_CONTACT_ENV_STEPS = 10


class _Recording(object):
    """The oracle with the collision masks of every step it takes kept (``_replay_through_oracle`` drops them)."""

    def __init__(self, oracle):
        self._o, self.colls = oracle, []

    def step(self, **kw):
        w = self._o.step(**kw)
        self.colls.append(w['coll'].copy())
        return w

    def __getattr__(self, name):
        return getattr(self._o, name)

    def contact_env_steps(self):
        """env-steps in which some agent's mask has a bit other than its own: an agent-agent contact."""
        N = self._o.N
        own = (np.uint64(1) << np.arange(N, dtype=np.uint64))[None, None, :]
        c = np.stack(self.colls)
        return int(((c & ~own) != 0).any(axis=2).sum())


def _spread(B, N, L=None, full=False, max_episode_len=25, seed=21, **kw):
    """-> (env, po_config) of one simple_spread configuration, canonical constants."""
    from multiagent_rl_amd import make_batched_env
    env = make_batched_env('simple_spread', B, n=N, num_landmarks=L, local_observation=not full, auto_reset=True,
                           max_episode_len=max_episode_len, seed=seed, **kw)
    cfg = co.make_config('simple_spread', N, num_landmarks=L, obs_mode='full' if full else 'local', max_episode_len=max_episode_len,
                         auto_reset=True, seed=seed)
    return env, cfg


def _oracle_parity(env, cfg, T, label, form5=False, contacts=True, desync=False, resets=None):
    """One launch of T steps replayed through the oracle; the actions against the float64 actor; a second launch of 3 steps from
    the stored state; the kernel's name.  -> the launch's outputs."""
    from multiagent_rl_amd.policy import ActorNetwork, FusedActor
    torch.manual_seed(4)
    B, N = env.num_envs, env.n
    if form5:
        env.set_dispatch(policy_form=5)
    o32 = _Recording(co.COracle(cfg, B, np.float32))
    actor = FusedActor(ActorNetwork(env.obs_dim, 5).cuda().eval(), seed=9)
    obs0 = o32.reset()
    _assert_same_bits(_np(env.reset()), obs0, 'reset obs')
    if desync:   # every env at another point of its episode: resets fall in different steps inside one wave
        es = (np.arange(B) % 25).astype(np.int32)
        env.set_state(o32.pos.copy(), o32.vel.copy(), o32.lm.copy(), ep_step=es, ep_count=o32.ep_count.astype(np.int32))
        o32.set_state(o32.pos.copy(), o32.vel.copy(), o32.lm.copy(), ep_step=es)
        _assert_same_bits(_np(env.observe()), obs0, 'obs after set_state')
    got = actor.rollout(env, T)
    assert env.last_kernel() == GENERIC, env.last_kernel()
    a = _np(got['act'])
    assert a.shape == (T, B, N) and a.dtype == np.int32 and a.min() >= 0 and a.max() <= 4
    assert len(np.unique(a)) == 5                       # a real policy sample, not a constant
    n_resets = _replay_through_oracle(o32, got, T)
    assert n_resets == (T // cfg.max_episode_len if resets is None else resets), n_resets
    _assert_final_state(env, o32)
    rows = np.concatenate([obs0[None], _np(got['obs'][:-1])], 0)
    assert_rollout_actions_match_f64(actor.actor, 9, 0, rows, a, label)
    n_contact = o32.contact_env_steps()
    print('%s: %d env-steps with an agent-agent contact' % (label, n_contact))
    # a second chunk continues from the stored state (and the oracle from its own)
    got2 = actor.rollout(env, 3)
    assert env.last_kernel() == GENERIC, env.last_kernel()
    _replay_through_oracle(o32, got2, 3)
    _assert_final_state(env, o32)
    rows2 = np.concatenate([_np(got['obs'][-1:]), _np(got2['obs'][:-1])], 0)
    assert_rollout_actions_match_f64(actor.actor, 9, T, rows2, _np(got2['act']), label + ' chunk 2')
    if contacts:
        assert n_contact >= MIN_CONTACT_ENV_STEPS, n_contact
    return got


def test_full_observation_smallest_rows_ragged_last_workgroup():
    """Case 1: full observation, N = L = 3 (D = 18), B = 37 = 2 x 16 + 5, 53 steps across two resets."""
    env, cfg = _spread(37, 3, full=True)
    assert env.obs_dim == 18
    _oracle_parity(env, cfg, 53, 'full N=3')


def test_full_observation_largest_rows_row_cap():
    """Case 2: full observation, N = L = 10 (D = 60, S1C = 8); E = 9 < 16 by the 96-row cap; B = 20: two full workgroups, a ragged third."""
    env, cfg = _spread(20, 10, full=True)
    assert env.obs_dim == 60 and env.lib.pw_policy_generic_envs_per_workgroup(0, 1, 10, 10, 0) == 9
    _oracle_parity(env, cfg, 27, 'full N=10')


def test_local_observation_more_landmarks_than_agents():
    """Case 3: local observation, N = 3, L = 5: the reward's per-landmark minimum goes through LDS (L > N)."""
    env, cfg = _spread(37, 3, L=5)
    assert env.obs_dim == 14
    _oracle_parity(env, cfg, 53, 'local N=3 L=5')


def test_more_than_one_environment_wave_per_workgroup():
    """Case 4: local observation, N = L = 12 under policy_form = 5: 8 environments per workgroup, 5 per wave -- two environment waves."""
    env, cfg = _spread(19, 12)
    assert env.lib.pw_policy_generic_envs_per_workgroup(0, 0, 12, 12, 0) == 8
    _oracle_parity(env, cfg, 27, 'local N=12 form 5', form5=True)


def test_idle_lanes_inside_an_environment_wave():
    """Case 5: N = L = 7 under policy_form = 5: 9 environments = 63 lanes per wave, lane 63 idle; 13 per workgroup."""
    env, cfg = _spread(29, 7)
    _oracle_parity(env, cfg, 27, 'local N=7 form 5', form5=True)


def test_heterogeneous_spread_agents_under_policy_form_5():
    """Case 6: the `mixed` constant set, simple_spread N = 5: per-agent size, acceleration, speed clamp and force scale."""
    env, cfg = _mk('mixed', 'simple_spread', 77, 5, max_episode_len=25, auto_reset=True, seed=13, want_coll=False, dispatch=dict(AUTO))
    _oracle_parity(env, cfg, 27, 'mixed spread N=5', form5=True)


def test_tag_roster_with_one_agent_unlike_its_role_under_policy_form_5():
    """Case 7: the `mixed` constant set, simple_tag 2 + 3: one good agent of another size."""
    env, cfg = _mk('mixed', 'simple_tag', 77, 5, A=2, max_episode_len=25, auto_reset=True, seed=13, want_coll=False, dispatch=dict(AUTO))
    got = _oracle_parity(env, cfg, 27, 'mixed tag 2+3', form5=True)
    assert float(got['rew'].abs().sum()) > 0


def test_heterogeneous_agents_stay_refused_under_automatic_dispatch():
    """Case 8: the handle of case 6 under automatic dispatch: PW_EINVAL, and the message says how to get it served."""
    from multiagent_rl_amd._lib import PworldError
    from multiagent_rl_amd.policy import ActorNetwork, FusedActor
    env, _ = _mk('mixed', 'simple_spread', 77, 5, max_episode_len=25, auto_reset=True, seed=13, want_coll=False, dispatch=dict(AUTO))
    env.reset()
    actor = FusedActor(ActorNetwork(env.obs_dim, 5).cuda().eval(), seed=9)
    with pytest.raises(PworldError, match='policy_form'):
        actor.rollout(env, 3)
    tag, _ = _mk('mixed', 'simple_tag', 20, 5, A=2, max_episode_len=25, auto_reset=True, seed=13, want_coll=False, dispatch=dict(AUTO))
    tag.reset()
    with pytest.raises(PworldError, match='policy_form'):
        FusedActor(ActorNetwork(tag.obs_dim, 5).cuda().eval(), seed=9).rollout(tag, 3)


def test_every_step_resets():
    """Case 9: max_episode_len = 1 -- every step ends an episode of every env."""
    env, cfg = _spread(20, 3, full=True, max_episode_len=1)
    _oracle_parity(env, cfg, 6, 'full N=3 len 1', contacts=False)


def test_desynchronised_episode_clocks():
    """Case 10: ep_step = arange(B) % 25 on env and oracle: in every step some env of a wave resets and its neighbours do not."""
    env, cfg = _spread(37, 3, full=True)
    _oracle_parity(env, cfg, 30, 'full N=3 desync', contacts=False, desync=True, resets=30)


# ---- HIP against HIP ----------------------------------------------------------------------------------------------------------

def _launch(env, net, T, seed=9):
    from multiagent_rl_amd.policy import FusedActor
    env.reset()
    got = FusedActor(net, seed=seed).rollout(env, T)
    return got, env.get_state(), env.last_kernel()


def _assert_same_launch(a, b, what):
    (ga, sa, _), (gb, sb, _) = a, b
    for key in ('obs', 'rew', 'rew_shared', 'terminal', 'done', 'act'):
        assert torch.equal(ga[key], gb[key]), '%s: %s differs' % (what, key)
    m = ga['terminal'].bool()
    assert m.any() and torch.equal(ga['final_obs'][m], gb['final_obs'][m]), '%s: final_obs differs' % what
    for key in ('pos', 'vel', 'landmarks', 'ep_step', 'ep_count'):
        assert torch.equal(sa[key], sb[key]), '%s: final %s differs' % (what, key)


def test_generic_form_equals_the_specialised_forms():
    """Case 11: on handles both serve, policy_form = 5 gives the bits of form 3 / the simple_tag kernel; a force_generic handle reaches
    the generic kernel under automatic dispatch with the same bits again."""
    from multiagent_rl_amd import make_batched_env
    from multiagent_rl_amd.policy import ActorNetwork
    torch.manual_seed(4)
    T = 53
    for scenario, B, kw, special in (('simple_spread', 100, dict(n=6), 'pw_policy_rollout3_kernel'),
                                     ('simple_tag', 37, dict(num_adversaries=4, num_good=2), 'pw_policy_rollout_tag_kernel')):
        mk = lambda **d: make_batched_env(scenario, B, auto_reset=True, max_episode_len=25, seed=21, **dict(kw, **d))  # noqa: E731
        env_s, env_g, env_f = mk(), mk(), mk(dispatch=dict(force_generic=1))
        net = ActorNetwork(env_s.obs_dim, 5).cuda().eval()
        env_g.set_dispatch(policy_form=5)
        ref = _launch(env_s, net, T)
        assert ref[2] == special, ref[2]
        for env, what in ((env_g, 'policy_form 5'), (env_f, 'force_generic')):
            out = _launch(env, net, T)
            assert out[2] == GENERIC, out[2]
            _assert_same_launch(ref, out, '%s %s' % (scenario, what))


def test_one_launch_equals_the_per_step_loop_and_fills_the_ring_like_collect():
    """Case 12: full observation N = 3, B = 37, T = 30.  The launch's outputs equal ``act = fused(obs); env.step(act)``; the ring the
    sink fills and the episode bookkeeping equal what BatchedRollout.collect leaves on a twin env (finished_sum up to float64
    summation order)."""
    from multiagent_rl_amd.policy import ActorNetwork, FusedActor
    from multiagent_rl_amd.replay_buffer import ReplayBuffer
    from multiagent_rl_amd.rollout import BatchedRollout
    torch.manual_seed(4)
    B, N, T = 37, 3, 30
    envs = [_spread(B, N, full=True)[0] for _ in range(3)]
    D = envs[0].obs_dim
    net = ActorNetwork(D, 5).cuda().eval()
    one = BatchedRollout(envs[0], FusedActor(net, seed=7), ReplayBuffer(B * 64, N, D))
    one.collect_one_launch(T, chunk=T, keep_outputs=True)
    assert envs[0].last_kernel() == GENERIC, envs[0].last_kernel()
    got = one.last_chunk
    # the per-step loop
    fused = FusedActor(net, seed=7)
    obs = envs[1].reset()
    for t in range(T):
        act = fused(obs)
        obs, rew, done, info = envs[1].step(act)
        assert torch.equal(got['act'][t], act), 'act[%d]' % t
        assert torch.equal(got['obs'][t], obs), 'obs[%d]' % t
        assert torch.equal(got['rew'][t], rew), 'rew[%d]' % t
        assert torch.equal(got['rew_shared'][t], info['rew_shared']), 'rew_shared[%d]' % t
        assert torch.equal(got['terminal'][t].bool(), info['terminal'].bool()), 'terminal[%d]' % t
        m = info['terminal'].bool()
        if m.any():
            assert torch.equal(got['final_obs'][t][m], info['final_obs'][m]), 'final_obs[%d]' % t
    # the ring and the bookkeeping
    loop = BatchedRollout(envs[2], FusedActor(net, seed=7), ReplayBuffer(B * 64, N, D))
    loop.collect(T)
    assert len(one.memory) == len(loop.memory) == T * B
    for plane in ('obs', 'act', 'rew', 'done', 'next_obs'):
        assert torch.equal(getattr(one.memory, plane)[:T * B], getattr(loop.memory, plane)[:T * B]), 'ring %s' % plane
    assert int(one.finished_episodes.item()) == int(loop.finished_episodes.item()) == B
    assert torch.equal(one.episode_return, loop.episode_return)
    s1, s2 = float(one.finished_return_sum.item()), float(loop.finished_return_sum.item())
    assert s2 != 0.0 and abs(s1 - s2) <= 1e-12 * abs(s2), (s1, s2)
    assert torch.equal(one.obs, loop.obs)


def test_sink_refusals():
    """Case 13: a STATE ring, a two-head ring, a ring of another obs_dim and the bf16x3 actor are each PW_EINVAL with a message."""
    from multiagent_rl_amd._lib import PworldError
    from multiagent_rl_amd.policy import ActorNetwork, FusedActor
    from multiagent_rl_amd.replay_buffer import ReplayBuffer
    env, _ = _spread(20, 3)                       # a fast-path handle: its STATE ring is a valid one
    env.set_dispatch(policy_form=5)
    env.reset()
    N, D = env.n, env.obs_dim
    actor = FusedActor(ActorNetwork(D, 5).cuda().eval(), seed=9)
    state = ReplayBuffer(4096, N, D, state_ring=dict(scenario='simple_spread', num_landmarks=3, num_adversaries=0))
    with pytest.raises(PworldError, match='STATE ring'):
        actor.rollout(env, 3, False, memory=state)
    with pytest.raises(PworldError, match='two-head'):
        actor.rollout(env, 3, False, memory=ReplayBuffer(4096, N, D, act_heads=(5, 10)))
    with pytest.raises(PworldError, match='shape mismatch'):
        actor.rollout(env, 3, False, memory=ReplayBuffer(4096, N, D + 2))
    env.set_actor_precision('bf16x3')
    with pytest.raises(PworldError, match='BF16X3'):
        actor.rollout(env, 3)
    env.set_actor_precision('f32')
    actor.rollout(env, 3, False, memory=ReplayBuffer(4096, N, D))       # and the plain row ring is served
    assert env.last_kernel() == GENERIC


def test_train_batched_on_a_full_observation_env(tmp_path):
    """Case 14: examples/train_batched.py --full-observation on cuda:0 (the pattern of tests/test_gpu_critic.py's entry test): two
    chunks of 25 steps on 64 envs finish 128 episodes."""
    sys.path.insert(0, os.path.join(ROOT, 'examples'))
    import train_batched as entry
    from multiagent_rl_amd import arglist
    saved = (arglist.num_episodes, arglist.save_rate, arglist.warmup_steps, arglist.batch_size)
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        arglist.warmup_steps, arglist.batch_size = 1024, 1024
        res = entry.main(['--scenario', 'simple_spread', '--envs', '64', '--agents', '3', '--full-observation', '--episodes', '128',
                          '--chunk', '25', '--save-rate', '64', '--max-updates-per-chunk', '1', '--out-dir', str(tmp_path / 'Models')])
    finally:
        os.chdir(cwd)
        arglist.num_episodes, arglist.save_rate, arglist.warmup_steps, arglist.batch_size = saved
    (name, cnt, st), = res
    assert name == 'simple_spread' and st['episodes'] == 128 and st['env_steps'] == 2 * 25 * 64, st
    assert (tmp_path / 'Models' / 'simple_spread_fin_0_actor.pt').exists()
