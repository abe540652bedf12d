"""GPU: the deferred step tail of the five one-launch policy rollout kernels (StepTail, csrc/pw_policy_shared.hpp) at its edge -- the
shortest launches, where the flush after the step loop and the reset path meet.

Each case is ONE pw_policy_rollout launch of T in {1, 2, 3} steps that carries both sinks (a row ring and the episode statistics) and
every step output, on B = 17 environments: two workgroups, the second ragged with a single environment.
  max_episode_len = 2: a deferred step (the tail runs inside the next actor pass, or in the flush when it was the last) is followed at
                       once by a resetting one (the tail runs in place, before the reset);
  max_episode_len = 0: no episode ever ends -- every step is deferred, the last one flushed.
The launch is compared bit for bit with the step loop the other equals-the-step-loop tests use (BatchedRollout.step: FusedActor() +
env.step() + the ring / statistics append), run once per (kernel, max_episode_len) for three steps and snapshotted after each.

finished_sum bit for bit: the step loop and the launch add the same finished returns, in float64, in different orders.  Every term is a
float32, and the test first checks that the sum of their magnitudes stays below 2^53 units of the smallest term's last place: then no
addition rounds, whatever the order, and the two sums must be the same bits.
"""
import functools
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

B = 17
STEPS = 3

# id -> (scenario, env kwargs, policy_form, actor heads, kernel)
KERNELS = {
    'form3': ('simple_spread', dict(n=3), 3, 5, 'pw_policy_rollout3_kernel'),
    'form4': ('simple_spread', dict(n=3), 4, 5, 'pw_policy_rollout3j_kernel'),
    'tag': ('simple_tag', dict(num_adversaries=2, num_good=1), 0, 5, 'pw_policy_rollout_tag_kernel'),
    'reference': ('simple_reference', dict(), 0, [5, 10], 'pw_policy_rollout_ref_kernel<3>'),
    'form5': ('simple_spread', dict(n=3), 5, 5, 'pw_policy_rollout_generic_kernel'),
}
STATE_KEYS = ('pos', 'vel', 'landmarks', 'ep_step', 'ep_count')
OUT_KEYS = ('obs', 'rew', 'rew_shared', 'terminal')
RING_KEYS = ('obs', 'next_obs', 'act', 'rew', 'done')


def _make(kernel, max_episode_len):
    from multiagent_rl_amd import make_batched_env
    from multiagent_rl_amd.policy import ActorNetwork, FusedActor
    from multiagent_rl_amd.replay_buffer import ReplayBuffer
    scenario, kw, form, heads, _ = KERNELS[kernel]
    env = make_batched_env(scenario, B, auto_reset=True, max_episode_len=max_episode_len, seed=21, **kw)
    if form:
        env.set_dispatch(policy_form=form)
    torch.manual_seed(4)
    actor = FusedActor(ActorNetwork(env.obs_dim, heads).cuda().eval(), seed=9)
    mem = ReplayBuffer(B * (STEPS + 1), env.n, env.obs_dim, act_heads=tuple(heads) if isinstance(heads, list) else None)
    return env, actor, mem


def _state(env):
    st = env.get_state()
    return {k: st[k].clone() for k in STATE_KEYS + (('comm', 'goal') if env.scenario_name == 'simple_reference' else ())}


def _ring(mem, rows):
    return {k: getattr(mem, k)[:rows].clone() for k in RING_KEYS}


@functools.lru_cache(maxsize=None)
def _step_loop(kernel, max_episode_len):
    """The reference, once per (kernel, max_episode_len): three steps of the step loop; -> per-step outputs and, after each step, the env
    state, the ring's filled rows and the statistics.  Callers only read it."""
    from multiagent_rl_amd.rollout import BatchedRollout
    env, actor, mem = _make(kernel, max_episode_len)
    ro = BatchedRollout(env, actor, mem)          # resets the env
    steps, after = [], []
    for t in range(STEPS):
        obs, rew, done, info = ro.step()
        assert not done.any()
        steps.append(dict(obs=obs.clone(), rew=rew.clone(), rew_shared=info['rew_shared'].clone(),
                          terminal=info['terminal'].clone(), final_obs=info['final_obs'].clone()))
        after.append(dict(state=_state(env), ring=_ring(mem, (t + 1) * B), cursor=mem._next_idx,
                          stats=(ro.episode_return.clone(), ro.finished_return_sum.clone(), ro.finished_episodes.clone())))
    return steps, after


def _sum_is_exact(terms):
    """No float64 addition of these float32 terms rounds, in any order: sum |terms| < 2^53 units of the smallest term's last place."""
    terms = [abs(float(x)) for x in terms if x != 0.0]
    if not terms:
        return True
    ulp = min(math.ldexp(1.0, math.frexp(x)[1] - 24) for x in terms)      # float32 last place of the smallest term
    return sum(terms) / ulp < 2.0 ** 53


@pytest.mark.parametrize('max_episode_len', [2, 0])
@pytest.mark.parametrize('T', [1, 2, 3])
@pytest.mark.parametrize('kernel', sorted(KERNELS))
def test_short_launch_with_both_sinks_equals_the_step_loop(kernel, T, max_episode_len):
    steps, after = _step_loop(kernel, max_episode_len)
    env, actor, mem = _make(kernel, max_episode_len)
    env.reset()
    stats = (torch.zeros(B, device='cuda'), torch.zeros((), dtype=torch.float64, device='cuda'),
             torch.zeros((), dtype=torch.int64, device='cuda'))
    got = actor.rollout(env, T, memory=mem, stats=stats)
    assert env.last_kernel() == KERNELS[kernel][4], env.last_kernel()
    want = {k: torch.stack([s[k] for s in steps[:T]]) for k in OUT_KEYS + ('final_obs',)}
    for k in OUT_KEYS:
        assert torch.equal(got[k], want[k]), k
    assert not got['done'].any()
    term = got['terminal']
    assert bool(term.any()) == (max_episode_len == 2 and T >= 2)      # the episode clocks: every env ends on every second step
    if term.any():
        assert torch.equal(got['final_obs'][term], want['final_obs'][term])
    ref = after[T - 1]
    # the sampled actions: the launch's act output against the ring the step loop filled (uint8 indices, [rows, N] or [rows, N, 2])
    assert torch.equal(got['act'].reshape(ref['ring']['act'].shape).to(torch.uint8), ref['ring']['act'])
    ring = _ring(mem, T * B)
    for k in RING_KEYS:
        assert torch.equal(ring[k], ref['ring'][k]), 'ring.' + k
    assert mem._next_idx == ref['cursor'] and len(mem) == T * B
    state = _state(env)
    for k in state:
        assert torch.equal(state[k], ref['state'][k]), k
    assert torch.equal(stats[0].view(torch.int32), ref['stats'][0].view(torch.int32)), 'episode_return'
    assert int(stats[2].item()) == int(ref['stats'][2].item()) == int(term.sum().item()), 'finished_count'
    # the finished returns: per env the sum of the episode's shared rewards, float32 additions in step order (run.py:55-65)
    rs = want['rew_shared'].cpu().numpy()
    ends = term.cpu().numpy().astype(bool)
    finished = [np.float32(rs[t - 1, e]) + np.float32(rs[t, e]) for t in range(T) for e in range(B) if ends[t, e]]
    assert _sum_is_exact(finished), 'the order of the float64 additions could show: the bit-for-bit comparison below is not justified'
    assert np.float64(stats[1].item()).view(np.uint64) == np.float64(ref['stats'][1].item()).view(np.uint64), 'finished_sum'
