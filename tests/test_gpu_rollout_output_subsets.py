"""GPU: pw_policy_rollout with a SUBSET of its outputs (include/pworld.h: with a sink -- a ring, the episode bookkeeping or both --
every output is optional; without one act_out, obs, rew, rew_shared, done and terminal are required).

All five one-launch kernel families guard every output store on its own (if (V.rew), if (V.obs), if (P.act_out) ...), and beside those
stores sit the sink's stores, the LDS observation row the next step's actor reads, and the episode bookkeeping.  A guard that encloses
one line too many is invisible while the only combinations ever run are "all outputs" and "none"; here every family runs with every
sink and, per sink, with the full set, with none (out=False), with each output alone, with the full set minus each, and with the four
names dist.py hands over -- against the full-set launch with the same kind of sink on a twin env and a twin actor (same weights, seed
and calls):

  * the outputs that were given are bit-identical, and nothing is written around them (tests/guarded.py);
  * the ring -- every plane whole, the slots the chunk does not reach included --, its cursor and its length are identical; a STATE
    ring also through sample_index over every filled slot;
  * the three statistics tensors are bit-identical (same kernel, same grid: the same float64 additions in the same order);
  * the env's state afterwards and the actor's step count are identical.

7 steps, episodes of 3 with auto-reset, rings of T * B + 5 slots with the cursor 5 before the end: the chunk wraps.  Without a sink, a
launch that leaves out one of the six required outputs is refused before anything runs.  No tolerance anywhere.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

from tests.guarded import assert_guards_intact, assert_untouched, guarded  # noqa: E402
from tests.test_gpu_parity import _assert_same_bits  # noqa: E402

T = 7
EP_LEN = 3
CALLS0 = 11            # the twin actors' step count before the launch: the Gumbel noise is keyed (seed; calls + t, row)
NAMES = ('obs', 'final_obs', 'rew', 'rew_shared', 'done', 'terminal', 'act')
REQUIRED = ('act', 'obs', 'rew', 'rew_shared', 'done', 'terminal')      # without a sink
DIST_NAMES = ('obs', 'rew_shared', 'final_obs', 'terminal')
SUBSETS = [NAMES, None] + [(x,) for x in NAMES] + [tuple(n for n in NAMES if n != x) for x in NAMES] + [DIST_NAMES]

# id -> (scenario, env kwargs, B, policy_form, actor heads, kernel, STATE ring description or None)
FAMILIES = {
    'spread6-form3': ('simple_spread', dict(n=6), 19, 3, 5, 'pw_policy_rollout3_kernel',
                      dict(scenario='simple_spread', num_landmarks=6, num_adversaries=0)),
    'spread6-form4': ('simple_spread', dict(n=6), 19, 4, 5, 'pw_policy_rollout3j_kernel',
                      dict(scenario='simple_spread', num_landmarks=6, num_adversaries=0)),
    'spread6-form5': ('simple_spread', dict(n=6), 19, 5, 5, 'pw_policy_rollout_generic_kernel', None),     # the generic form: row rings only
    # Automatic dispatch takes the just-in-time form where the plain third form cannot keep min(B, 16) environments in one workgroup:
    # its LDS (roll3_lds: 128 N^2 + 9 K N + 21 K bytes at 16 environments) passes 160 KB between N = 13 and N = 14, where 13 environments
    # fit.  So N = 13 stays on the third form at any B (here with run-time N, unlike the N = 6 case above), and N = 14 at B = 17 -- two
    # workgroups, the second with a single environment -- is the smallest shape that reaches the just-in-time form unforced.
    'spread13-auto': ('simple_spread', dict(n=13), 5, 0, 5, 'pw_policy_rollout3_kernel',
                      dict(scenario='simple_spread', num_landmarks=13, num_adversaries=0)),
    'spread14-auto': ('simple_spread', dict(n=14), 17, 0, 5, 'pw_policy_rollout3j_kernel',
                      dict(scenario='simple_spread', num_landmarks=14, num_adversaries=0)),
    'tag3+1-auto': ('simple_tag', dict(num_adversaries=3, num_good=1), 10, 0, 5, 'pw_policy_rollout_tag_kernel',
                    dict(scenario='simple_tag', num_landmarks=2, num_adversaries=3)),
    'tag3+1-form5': ('simple_tag', dict(num_adversaries=3, num_good=1), 10, 5, 5, 'pw_policy_rollout_generic_kernel', None),
    'reference': ('simple_reference', dict(), 17, 0, [5, 10], 'pw_policy_rollout_ref_kernel<3>', None),    # two heads, act_heads=(5, 10) ring
}
SINKS = ('ring', 'state', 'stats', 'ring+stats')
PAIRS = [(f, s) for f in sorted(FAMILIES) for s in SINKS if s != 'state' or FAMILIES[f][6] is not None]


def _np(t):
    return t.detach().cpu().numpy()


def _sid(sub):
    if sub is None:
        return 'out=False'
    if sub == NAMES:
        return 'all'
    if len(sub) == len(NAMES) - 1:
        return 'all-but-' + [n for n in NAMES if n not in sub][0]
    return '+'.join(sub)


@functools.lru_cache(maxsize=None)
def _network(family):
    """The actor's module, built once per family (only read afterwards: every launch snapshots it into its own FusedActor)."""
    from multiagent_rl_amd import make_batched_env
    from multiagent_rl_amd.policy import ActorNetwork
    scenario, kw, B, _, heads, _, _ = FAMILIES[family]
    D = make_batched_env(scenario, B, **kw).obs_dim
    torch.manual_seed(4)
    return ActorNetwork(D, heads).cuda().eval()


def _twin(family):
    from multiagent_rl_amd import make_batched_env
    from multiagent_rl_amd.policy import FusedActor
    scenario, kw, B, form, _, _, _ = FAMILIES[family]
    env = make_batched_env(scenario, B, auto_reset=True, max_episode_len=EP_LEN, seed=21, env_id_base=3, **kw)
    if form:
        env.set_dispatch(policy_form=form)
    env.reset()
    actor = FusedActor(_network(family), seed=9)
    actor.calls = CALLS0
    return env, actor


def _ring(family, env, sink):
    """A ring of T * B + 5 slots, every plane pre-filled, the cursor 5 before the end (the chunk wraps), or None."""
    from multiagent_rl_amd.replay_buffer import ReplayBuffer
    if sink not in ('ring', 'state', 'ring+stats'):
        return None
    heads, state = FAMILIES[family][4], FAMILIES[family][6]
    cap = T * env.num_envs + 5
    mem = ReplayBuffer(cap, env.n, env.obs_dim, act_heads=tuple(heads) if isinstance(heads, list) else None,
                       state_ring=state if sink == 'state' else None)
    for k in _ring_keys(mem):
        plane = getattr(mem, k)
        plane.copy_((torch.arange(plane.numel(), device=plane.device) % 251).reshape(plane.shape).to(plane.dtype))
    mem._next_idx, mem._len = cap - 5, 0
    return mem


def _ring_keys(mem):
    return ('obs', 'next_obs', 'act', 'rew', 'done') + (('lm',) if mem.state_ring else ())


def _stats(env, sink):
    """(episode_return [B], finished_sum, finished_count) with a carry-in, in guarded buffers, or None."""
    if 'stats' not in sink:
        return None
    ret, fsum, fcnt = guarded((env.num_envs,), torch.float32), guarded((1,), torch.float64), guarded((1,), torch.int64)
    ret.copy_(torch.arange(env.num_envs, device='cuda', dtype=torch.float32) * 0.125 - 1.0)
    fsum.fill_(3.5)
    fcnt.fill_(2)
    return ret, fsum, fcnt


def _alloc(family, env, sub):
    if sub is None:
        return False
    B, N, D = env.num_envs, env.n, env.obs_dim
    two = isinstance(FAMILIES[family][4], list)
    shapes = dict(obs=(T, B, N, D), final_obs=(T, B, N, D), rew=(T, B, N), rew_shared=(T, B), done=(T, B, N), terminal=(T, B),
                  act=(T, B, N, 2) if two else (T, B, N))
    dtypes = dict(obs=torch.float32, final_obs=torch.float32, rew=torch.float32, rew_shared=torch.float32, done=torch.bool,
                  terminal=torch.bool, act=torch.int32)
    out = {n: guarded(shapes[n], dtypes[n]) for n in sub}
    out.setdefault('act', None)      # None: the launch gets act_out = NULL (an absent key would be allocated by FusedActor.rollout)
    return out


def _state(env):
    return {k: _np(v) for k, v in env.get_state().items()}


def _launch(family, sink, sub):
    """One pw_policy_rollout launch on a fresh twin -> everything it left behind, as numpy."""
    env, actor = _twin(family)
    mem, stats = _ring(family, env, sink), _stats(env, sink)
    out = _alloc(family, env, sub)
    actor.rollout(env, T, out=out, memory=mem, stats=stats)
    torch.cuda.synchronize()
    kernel = env.last_kernel()
    assert kernel == FAMILIES[family][5], kernel
    what = '%s, sink %s, outputs %s' % (family, sink, _sid(sub))
    got = dict(out={}, kernel=kernel, calls=actor.calls, state=_state(env))
    for n, t in (out or {}).items():
        if t is not None:
            assert_guards_intact(t, '%s: %s' % (what, n))
            got['out'][n] = _np(t)
    if mem is not None:
        got['ring'] = {k: _np(getattr(mem, k)) for k in _ring_keys(mem)}
        got['cursor'], got['len'] = mem._next_idx, len(mem)
        if mem.state_ring:      # the rows a learner would draw: rebuilt from the states, over every filled slot
            cap = mem._maxsize
            filled = list(range(cap - 5, cap)) + list(range(0, T * env.num_envs - 5))
            got['sample'] = [_np(x) for x in mem.sample_index(filled)]
    if stats is not None:
        for n, t in zip(('episode_return', 'finished_sum', 'finished_count'), stats):
            assert_guards_intact(t, '%s: %s' % (what, n))
        got['stats'] = [_np(t) for t in stats]
    return got


@functools.lru_cache(maxsize=None)
def _full(family, sink):
    return _launch(family, sink, NAMES)


@pytest.mark.parametrize('family, sink', PAIRS, ids=['%s-%s' % p for p in PAIRS])
def test_every_output_subset_leaves_what_the_full_set_leaves(family, sink):
    want = _full(family, sink)
    B = FAMILIES[family][2]
    # the reference launch itself did something: two resets inside the chunk, the ring wrapped, the statistics moved
    term = want['out']['terminal']
    assert term[[2, 5]].all() and not term[[0, 1, 3, 4, 6]].any()
    assert not want['out']['done'].any()
    if 'ring' in want:
        assert want['cursor'] == T * B - 5 and want['len'] == T * B
    if 'stats' in want:
        assert int(want['stats'][2][0]) == 2 + 2 * B and float(want['stats'][1][0]) != 3.5
    for sub in SUBSETS:
        got = _launch(family, sink, sub)
        what = '%s, sink %s, outputs %s [%s]' % (family, sink, _sid(sub), got['kernel'])
        assert sorted(got['out']) == sorted(sub or ()), what
        for n in got['out']:      # whole buffers: final_obs rows of steps without a reset keep the guard pattern in both
            _assert_same_bits(got['out'][n], want['out'][n], '%s: %s' % (what, n))
        assert ('ring' in got) == ('ring' in want) and ('stats' in got) == ('stats' in want), what
        if 'ring' in want:
            for k in want['ring']:
                _assert_same_bits(got['ring'][k], want['ring'][k], '%s: ring.%s' % (what, k))
            assert (got['cursor'], got['len']) == (want['cursor'], want['len']), what
        if 'sample' in want:
            for i, name in enumerate(('obs', 'act', 'rew', 'next_obs', 'done')):
                _assert_same_bits(got['sample'][i], want['sample'][i], '%s: sample_index %s' % (what, name))
        if 'stats' in want:
            _assert_same_bits(got['stats'][0], want['stats'][0], what + ': episode_return')
            assert got['stats'][1].view(np.uint64)[0] == want['stats'][1].view(np.uint64)[0], what + ': finished_sum'
            assert got['stats'][2][0] == want['stats'][2][0], what + ': finished_count'
        assert sorted(got['state']) == sorted(want['state']), what
        for k in want['state']:
            _assert_same_bits(got['state'][k], want['state'][k], '%s: state.%s afterwards' % (what, k))
        assert got['calls'] == want['calls'] == CALLS0 + T, what


@pytest.mark.parametrize('family', sorted(FAMILIES))
def test_the_row_ring_and_the_state_ring_hold_the_same_transitions(family):
    """What anchors the rings' contents on the outputs: the row ring's planes are the chunk's own outputs in slot order, and a STATE
    ring samples to the same rows."""
    want = _full(family, 'ring')
    B = FAMILIES[family][2]
    cap = T * B + 5
    slots = (cap - 5 + np.arange(T * B)) % cap
    out, ring = want['out'], want['ring']
    N = out['obs'].shape[2]
    _assert_same_bits(ring['next_obs'][slots].reshape(T, B, N, -1)[~out['terminal']], out['obs'][~out['terminal']], 'next_obs = obs')
    _assert_same_bits(ring['next_obs'][slots].reshape(T, B, N, -1)[out['terminal']], out['final_obs'][out['terminal']],
                      'next_obs = the pre-reset row where the episode ended')
    _assert_same_bits(ring['obs'][slots].reshape(T, B, N, -1)[1:], out['obs'][:-1], 'obs = the row acted on')
    _assert_same_bits(ring['rew'][slots].reshape(T, B), out['rew_shared'], 'rew')
    assert np.array_equal(ring['act'][slots].reshape(out['act'].shape), out['act'].astype(np.uint8)) and not ring['done'][slots].any()
    if FAMILIES[family][6] is not None:
        st = _full(family, 'state')
        idx = list(range(cap - 5, cap)) + list(range(0, T * B - 5))
        _assert_same_bits(st['sample'][0], ring['obs'][idx], 'STATE ring: sampled obs')
        _assert_same_bits(st['sample'][3], ring['next_obs'][idx], 'STATE ring: sampled next_obs')
        _assert_same_bits(st['sample'][2], ring['rew'][idx], 'STATE ring: sampled rew')


@pytest.mark.parametrize('left_out', REQUIRED)
@pytest.mark.parametrize('family', sorted(FAMILIES))
def test_without_a_sink_a_missing_required_output_is_refused_before_the_launch(family, left_out):
    from multiagent_rl_amd._lib import PworldError
    env, actor = _twin(family)
    before = _state(env)
    out = _alloc(family, env, tuple(n for n in NAMES if n != left_out))      # act left out: out['act'] = None
    with pytest.raises(PworldError, match='without a sink'):
        actor.rollout(env, T, out=out)
    torch.cuda.synchronize()
    assert actor.calls == CALLS0 and env.last_kernel() == ''
    after = _state(env)
    for k in before:
        _assert_same_bits(after[k], before[k], '%s without %s: state.%s' % (family, left_out, k))
    for n, t in out.items():      # the decoys: nothing reached any buffer that was handed over
        if t is not None:
            assert_untouched(t, '%s without %s: %s' % (family, left_out, n))


@pytest.mark.parametrize('family', sorted(FAMILIES))
def test_a_sink_that_takes_nothing_is_no_sink(family):
    """A pw_rollout_sink with neither a ring nor episode_return is refused like no sink at all when outputs are missing; the
    statistics alone (FusedActor.rollout(out=False, stats=...)) are a sink."""
    import ctypes as C
    from multiagent_rl_amd import _lib
    env, actor = _twin(family)
    io, sink, p = _lib.PwStepIO(), _lib.PwRolloutSink(), _lib.ptr
    rc = actor.lib.pw_policy_rollout(env._h, p(actor.frag), p(actor.b1), p(actor.bih), p(actor.whh_f), p(actor.whh_r), p(actor.w2),
                                     p(actor.b2), 1, actor.seed, actor.calls, None, C.byref(io), None, T, C.byref(sink),
                                     _lib.stream(actor.device))
    assert rc == -1 and b'without a sink' in actor.lib.pw_last_error() and env.last_kernel() == ''
    stats = _stats(env, 'stats')
    actor.rollout(env, T, out=False, stats=stats)
    assert env.last_kernel() == FAMILIES[family][5] and int(stats[2][0]) == 2 + 2 * FAMILIES[family][2]
