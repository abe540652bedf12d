"""GPU: the ring sink of pw_policy_rollout into a PER-AGENT ring (pw_replay_store.per_agent: rew / done [cap, N], the BiCNet tuple of
experiments/run_BIC.py:46,50), in every form of the launch and for each kind of ring the form takes, and the per-agent STATE ring.

The shapes are those of tests/test_gpu_rollout_output_subsets.py (its FAMILIES: every kernel family, compile-time and run-time N, a
second workgroup with one environment): 7 steps, episodes of 3 with auto-reset, rings of T * B + 5 slots with the cursor 5 before the
end (the chunk wraps), a non-zero env_id_base.  Every launch runs on a fresh twin env and twin actor (same weights, seed and step
count), and every comparison is on bits:

  1. the sink stores what the two-launch path stored: the rollout with all outputs followed by ReplayBuffer.add_rollout (what
     tests/test_gpu_bicnet.py ties to T add_batch calls) -- all planes over all slots, the env's state, the statistics; and the ring's
     rew plane is the launch's own out['rew'] in slot order;
  2. leaving every output out changes no ring plane, no statistic and not the state;
  3. a per-agent STATE ring samples to the per-agent row ring's batch, through pw_replay_gather and through pw_replay_sample;
  4. the shared row ring of a twin launch holds the same obs / next_obs / act, and its rew is out['rew_shared'];
  5. collect_one_launch with a per-agent memory is one launch per chunk (torch.profiler);
  6. pw_policy_rollout through ctypes takes a per-agent row ring, STATE ring and two-head ring, and ReplayBuffer builds the STATE one;
  7. the tail / packed / wire entry points, a ring of the wrong number of heads and a STATE ring on the generic form or of another
     shape stay PW_EINVAL, with the ring (in guarded buffers, tests/guarded.py) untouched;
  8. examples/train_batched.py --critic bicnet trains to the same four losses on its STATE ring as on the row ring.
"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

from tests.guarded import assert_guards_intact, assert_untouched, guarded  # noqa: E402
from tests.test_gpu_parity import _assert_same_bits  # noqa: E402
from tests.test_gpu_rollout_output_subsets import CALLS0, FAMILIES, NAMES, T, _alloc, _np, _ring_keys, _state, _stats, _twin  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = sorted(FAMILIES)
WITH_STATE = [f for f in ALL if FAMILIES[f][6] is not None]      # the first five and tag3+1-auto
KINDS = [(f, k) for f in ALL for k in ('rows', 'state') if k == 'rows' or f in WITH_STATE]
KIND_IDS = ['%s-%s' % p for p in KINDS]


def _ring(family, env, kind, per_agent=True, **kw):
    """A ring of T * B + 5 slots, every plane holding a sentinel, the cursor 5 before the end (the chunk wraps)."""
    from multiagent_rl_amd.replay_buffer import ReplayBuffer
    heads, state = FAMILIES[family][4], FAMILIES[family][6]
    cap = T * env.num_envs + 5
    mem = ReplayBuffer(cap, env.n, env.obs_dim, act_heads=tuple(heads) if isinstance(heads, list) else None, per_agent=per_agent,
                       state_ring=state if kind == 'state' else None, **kw)
    assert tuple(mem.rew.shape) == tuple(mem.done.shape) == ((cap, env.n) if per_agent else (cap,))
    for k in _ring_keys(mem):
        plane = getattr(mem, k)
        plane.copy_(_sentinel(plane))
    mem._next_idx, mem._len = cap - 5, 0
    return mem


def _sentinel(plane):
    return (torch.arange(plane.numel(), device=plane.device) % 251).reshape(plane.shape).to(plane.dtype)


def _slots(B):
    cap = T * B + 5
    return (cap - 5 + np.arange(T * B)) % cap       # slot of transition (t, env), t-major: the order of T add_batch calls


def _launch(family, kind, sub, per_agent=True):
    """One launch with the ring as its sink on a fresh twin -> what it left behind, as numpy (and the ring itself)."""
    env, actor = _twin(family)
    mem, stats = _ring(family, env, kind, per_agent), _stats(env, 'stats')
    out = _alloc(family, env, sub)
    actor.rollout(env, T, out=out, memory=mem, stats=stats)
    torch.cuda.synchronize()
    assert env.last_kernel() == FAMILIES[family][5], env.last_kernel()
    what = '%s, %s ring, outputs %s' % (family, kind, 'all' if sub else 'none')
    for n, t in list((out or {}).items()) + list(zip(('episode_return', 'finished_sum', 'finished_count'), stats)):
        if t is not None:
            assert_guards_intact(t, '%s: %s' % (what, n))
    assert (mem._next_idx, len(mem), actor.calls) == (T * env.num_envs - 5, T * env.num_envs, CALLS0 + T)
    return dict(out={n: _np(t) for n, t in (out or {}).items() if t is not None}, ring={k: _np(getattr(mem, k)) for k in _ring_keys(mem)},
                stats=[_np(t) for t in stats], state=_state(env), mem=mem)


@functools.lru_cache(maxsize=None)
def _full(family, kind, per_agent=True):
    return _launch(family, kind, NAMES, per_agent)


@functools.lru_cache(maxsize=None)
def _two_launches(family):
    """The parent's path: the rollout with all outputs and the statistics sink, then ReplayBuffer.add_rollout into a per-agent row ring."""
    env, actor = _twin(family)
    mem, stats = _ring(family, env, 'rows'), _stats(env, 'stats')
    obs0 = env.observe().clone()
    out = _alloc(family, env, NAMES)
    actor.rollout(env, T, out=out, stats=stats)
    mem.add_rollout(obs0, out)
    torch.cuda.synchronize()
    assert env.last_kernel() == FAMILIES[family][5], env.last_kernel()
    return dict(ring={k: _np(getattr(mem, k)) for k in _ring_keys(mem)}, stats=[_np(t) for t in stats], state=_state(env),
                cursor=(mem._next_idx, len(mem)))


def _same_run(got, want, what):
    """Ring planes (all slots), statistics and the env's state afterwards, bit for bit."""
    assert sorted(got['ring']) == sorted(want['ring']), what
    for k in want['ring']:
        _assert_same_bits(got['ring'][k], want['ring'][k], '%s: ring.%s' % (what, k))
    _assert_same_bits(got['stats'][0], want['stats'][0], what + ': episode_return')
    assert got['stats'][1].view(np.uint64)[0] == want['stats'][1].view(np.uint64)[0], what + ': finished_sum'
    assert got['stats'][2][0] == want['stats'][2][0], what + ': finished_count'
    assert sorted(got['state']) == sorted(want['state']), what
    for k in want['state']:
        _assert_same_bits(got['state'][k], want['state'][k], '%s: state.%s afterwards' % (what, k))


# ---- 1. the sink stores what the two-launch path stored


@pytest.mark.parametrize('family', ALL)
def test_the_sink_stores_what_rollout_plus_add_rollout_stored(family):
    want, got = _two_launches(family), _full(family, 'rows')
    B = FAMILIES[family][2]
    cap, slots = T * B + 5, _slots(B)
    assert want['cursor'] == (T * B - 5, T * B)
    assert int(got['stats'][2][0]) == 2 + 2 * B            # two resets inside the chunk
    _same_run(got, want, family)
    N = got['out']['rew'].shape[2]
    untouched = np.arange(T * B - 5, T * B)                # the five slots the chunk does not reach keep the sentinel
    for k, plane in got['ring'].items():
        sent = _np(_sentinel(getattr(got['mem'], k)))
        _assert_same_bits(plane[untouched], sent[untouched], '%s: ring.%s outside the chunk' % (family, k))
    assert got['ring']['rew'].shape == (cap, N) and got['ring']['done'].shape == (cap, N)
    _assert_same_bits(got['ring']['rew'][slots].reshape(T, B, N), got['out']['rew'], family + ": ring.rew = the launch's own rew")
    assert not got['ring']['done'][slots].any() and not got['out']['done'].any()
    if family.startswith('tag'):       # adversaries and the good agent are rewarded differently: the planes really are per agent
        rew = got['ring']['rew'][slots]
        assert not np.array_equal(rew, np.broadcast_to(rew[:, :1], rew.shape))


# ---- 2. leaving outputs out changes nothing


@pytest.mark.parametrize('family, kind', KINDS, ids=KIND_IDS)
def test_every_output_left_out_leaves_the_same_ring_state_and_statistics(family, kind):
    got = _launch(family, kind, None)
    assert not got['out']
    _same_run(got, _full(family, kind), '%s, %s ring, out=False' % (family, kind))


# ---- 3. a per-agent STATE ring samples to the per-agent row ring's batch


@pytest.mark.parametrize('family', WITH_STATE)
def test_a_per_agent_state_ring_samples_to_the_row_rings_batch(family):
    rows, state = _full(family, 'rows'), _full(family, 'state')
    B = FAMILIES[family][2]
    N = rows['out']['rew'].shape[2]
    for k in ('act', 'rew', 'done'):       # the planes the two kinds share
        _assert_same_bits(state['ring'][k], rows['ring'][k], '%s: ring.%s' % (family, k))
    assert state['ring']['obs'].shape[2] == 4 and state['mem'].state_ring and state['mem'].per_agent
    idx = [int(s) for s in _slots(B)]
    want, got = rows['mem'].sample_index(idx), state['mem'].sample_index(idx)
    assert tuple(got[2].shape) == tuple(got[4].shape) == (T * B, N)
    for name, g, w in zip(('obs', 'act', 'rew', 'next_obs', 'done'), got, want):
        _assert_same_bits(_np(g), _np(w), '%s: sample_index %s' % (family, name))
    _assert_same_bits(_np(got[2]).reshape(T, B, N), rows['out']['rew'], family + ': sampled rew = the launch\'s rew')


@pytest.mark.parametrize('family', WITH_STATE)
def test_a_per_agent_state_ring_draws_and_gathers_in_one_launch(family):
    """pw_replay_sample (ReplayBuffer(device_index='counter')) on the STATE ring, on its own drawn slots, against pw_replay_gather on the
    row ring at those slots.  The length is set to the T * B - 5 slots at the ring's start, all of them filled."""
    rows = _full(family, 'rows')
    B = FAMILIES[family][2]
    env, actor = _twin(family)
    mem = _ring(family, env, 'state', device_index='counter', index_seed=5)
    actor.rollout(env, T, out=False, memory=mem)
    assert env.last_kernel() == FAMILIES[family][5]
    mem._len = T * B - 5
    b = 48
    idx = mem.make_index(b)
    mem.reset_draws(0)
    got = mem.sample(b)                    # the same draw number: the same slots
    assert tuple(idx.shape) == (b,) and int(idx.min()) >= 0 and int(idx.max()) < T * B - 5 and len(set(idx.tolist())) > 1
    want = rows['mem'].sample_index(idx)
    assert tuple(got[2].shape) == tuple(got[4].shape) == (b, env.n)
    for name, g, w in zip(('obs', 'act', 'rew', 'next_obs', 'done'), got, want):
        _assert_same_bits(_np(g), _np(w), '%s: sample %s' % (family, name))


def test_a_per_agent_state_ring_pickles_and_keeps_refusing_rows():
    import pickle
    from multiagent_rl_amd._lib import PworldError
    family = 'tag3+1-auto'
    got = _full(family, 'state')
    mem, B = got['mem'], FAMILIES[family][2]
    planes = mem.host_planes()
    assert planes['rew'].shape == planes['done'].shape == (T * B, 4) and planes['obs'].shape == (T * B, 4, 4)
    twin = pickle.loads(pickle.dumps(mem))
    assert twin.per_agent is True and twin.state_ring == mem.state_ring and len(twin) == len(mem)
    idx = list(range(T * B - 5))
    for g, w in zip(twin.sample_index(idx), mem.sample_index(idx)):
        _assert_same_bits(_np(g), _np(w), 'unpickled per-agent STATE ring')
    assert tuple(twin.rew.shape) == tuple(mem.rew.shape)
    env, _ = _twin(family)
    obs = env.observe()
    with pytest.raises(PworldError, match='STATE ring'):
        mem.add_batch(obs, torch.zeros(B, 4, dtype=torch.int32, device='cuda'), torch.zeros(B, 4, device='cuda'), obs)
    with pytest.raises(PworldError, match='STATE ring'):
        mem.add_rollout(obs, {k: torch.from_numpy(v).cuda() for k, v in got['out'].items()})


# ---- 4. the shared rings are untouched


@pytest.mark.parametrize('family', ['spread6-form3', 'tag3+1-auto'])
def test_the_shared_ring_of_a_twin_launch_holds_the_same_rows_and_the_shared_reward(family):
    pa, sh = _full(family, 'rows'), _full(family, 'rows', False)
    B = FAMILIES[family][2]
    slots = _slots(B)
    for k in ('obs', 'next_obs', 'act'):
        _assert_same_bits(sh['ring'][k], pa['ring'][k], '%s: ring.%s' % (family, k))
    assert sh['ring']['rew'].shape == (T * B + 5,)
    _assert_same_bits(sh['ring']['rew'][slots].reshape(T, B), pa['out']['rew_shared'], family + ': shared ring.rew = rew_shared')
    assert not sh['ring']['done'][slots].any()
    for k in sh['out']:
        _assert_same_bits(sh['out'][k], pa['out'][k], '%s: out.%s' % (family, k))


# ---- 5. one launch per chunk


def test_collect_one_launch_with_a_per_agent_memory_is_one_launch_per_chunk():
    from torch.profiler import ProfilerActivity, profile
    from multiagent_rl_amd import make_batched_env
    from multiagent_rl_amd.policy import ActorNetwork, FusedActor
    from multiagent_rl_amd.replay_buffer import ReplayBuffer
    from multiagent_rl_amd.rollout import BatchedRollout
    torch.manual_seed(0)
    env = make_batched_env('simple_spread', 8, auto_reset=True, max_episode_len=5, seed=11, n=3)
    mem = ReplayBuffer(64, env.n, env.obs_dim, per_agent=True)
    ro = BatchedRollout(env, FusedActor(ActorNetwork(env.obs_dim, 5).cuda().eval(), seed=7), mem)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        ro.collect_one_launch(12, chunk=5)
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if str(getattr(e, 'device_type', '')).endswith('CUDA')]
    assert sum('pw_policy_rollout' in n for n in names) == 3, names        # chunks of 5, 5 and 2 steps
    assert not [n for n in names if 'pw_replay_add_rollout' in n], names
    assert len(mem) == 64 and mem._next_idx == (12 * 8) % 64 and ro.stats()['episodes'] == 2 * 8


# ---- 6. what the library refused before


def _raw_rollout(env, actor, mem):
    """pw_policy_rollout through ctypes, every output NULL, the ring as the only sink -> return code."""
    from multiagent_rl_amd import _lib
    io, sink, p = _lib.PwStepIO(), _lib.PwRolloutSink(), _lib.ptr
    sink.ring, sink.ring_start = C.addressof(mem._store), mem._next_idx
    return actor.lib.pw_policy_rollout(env._h, p(actor.frag), p(actor.b1), p(actor.bih), p(actor.whh_f), p(actor.whh_r), p(actor.w2),
                                       p(actor.b2), 1, actor.seed, actor.calls, None, C.byref(io), None, T, C.byref(sink),
                                       _lib.stream(actor.device))


@pytest.mark.parametrize('family, kind', [('spread6-form3', 'rows'), ('spread6-form3', 'state'), ('reference', 'rows')],
                         ids=['row-ring', 'STATE-ring', 'two-head-ring'])
def test_pw_policy_rollout_takes_a_per_agent_sink(family, kind):
    env, actor = _twin(family)
    mem = _ring(family, env, kind)
    assert mem._store.per_agent == 1 and mem._store.state_rows == (kind == 'state') and mem._store.act_heads == (2 if family == 'reference' else 1)
    rc = _raw_rollout(env, actor, mem)
    torch.cuda.synchronize()
    assert rc == 0, actor.lib.pw_last_error()
    assert env.last_kernel() == FAMILIES[family][5]
    _assert_same_bits(_np(mem.rew), _full(family, kind)['ring']['rew'], '%s, %s ring through ctypes' % (family, kind))


def test_replay_buffer_builds_a_per_agent_state_ring():
    from multiagent_rl_amd.replay_buffer import ReplayBuffer
    mem = ReplayBuffer(8, 3, 10, per_agent=True, state_ring=dict(scenario='simple_spread', num_landmarks=3, num_adversaries=0))
    assert tuple(mem.rew.shape) == (8, 3) and tuple(mem.done.shape) == (8, 3) and tuple(mem.obs.shape) == (8, 3, 4)
    assert mem._store.per_agent == 1 and mem._store.state_rows == 1
    with pytest.raises(ValueError, match='single-head'):
        ReplayBuffer(8, 2, 21, per_agent=True, act_heads=(5, 10), state_ring=dict(scenario='simple_spread', num_landmarks=3))


# ---- 7. what stays refused


def _guard_ring(mem):
    """Move the ring's planes into guarded buffers (same contents) and point the store at them."""
    for k in _ring_keys(mem):
        plane = getattr(mem, k)
        g = guarded(plane.shape, plane.dtype)
        g.copy_(_sentinel(plane))
        setattr(mem, k, g)
        setattr(mem._store, k, g.data_ptr())
    return mem


def _ring_untouched(mem, what):
    torch.cuda.synchronize()
    for k in _ring_keys(mem):
        plane = getattr(mem, k)
        assert_guards_intact(plane, '%s: ring.%s' % (what, k))
        assert torch.equal(plane, _sentinel(plane)), '%s: ring.%s was written' % (what, k)


def test_the_tail_packed_and_wire_entry_points_refuse_a_per_agent_ring():
    from multiagent_rl_amd import _lib
    lib = _lib.load()
    EINVAL = -1
    family = 'tag3+1-auto'
    env, _ = _twin(family)
    B, N, D = env.num_envs, env.n, env.obs_dim
    buf = torch.zeros(1 << 20, dtype=torch.uint8, device='cuda')       # stands in for every input: nothing may be read or launched
    p = C.c_void_p(buf.data_ptr())
    for kind in ('rows', 'state'):
        mem = _guard_ring(_ring(family, env, kind))
        st = C.byref(mem._store)
        what = 'per-agent %s ring' % kind
        assert lib.pw_replay_add_tail(st, 0, None, None, B, p, p, p, p, p, p, None, p, p, p, None, None) == EINVAL, what
        assert b'pw_replay_add_tail' in lib.pw_last_error() and (b'per-agent' in lib.pw_last_error()), lib.pw_last_error()
        assert lib.pw_replay_add_packed(st, 0, 4, p, None) == EINVAL and b'per-agent' in lib.pw_last_error(), what
        cw = _lib.PwChunkWire()
        assert lib.pw_chunk_wire_layout(T, B, N, D, 3, C.byref(cw)) == 0 and cw.total_bytes <= buf.numel()
        assert lib.pw_replay_add_wire(st, 0, C.byref(cw), p, None) == EINVAL and b'per-agent' in lib.pw_last_error(), what
        sw = _lib.PwStateWire()
        assert lib.pw_state_wire_layout_scn(_lib.PW_SIMPLE_TAG, T, B, N, 2, 3, 3, C.byref(sw)) == 0 and sw.total_bytes <= buf.numel()
        assert lib.pw_replay_add_state_wire(st, 0, C.byref(sw), p, None) == EINVAL, (what, lib.pw_last_error())
        assert b'pw_replay_add_state_wire' in lib.pw_last_error() and b'per-agent' in lib.pw_last_error(), lib.pw_last_error()
        _ring_untouched(mem, what)
    env2, _ = _twin('reference')
    mem = _guard_ring(_ring('reference', env2, 'rows'))
    rw = _lib.PwRefWire()
    assert lib.pw_ref_wire_layout(T, env2.num_envs, 3, C.byref(rw)) == 0 and rw.total_bytes <= buf.numel()
    assert lib.pw_replay_add_ref_wire(C.byref(mem._store), 0, C.byref(rw), p, None) == EINVAL
    assert b'pw_replay_add_ref_wire' in lib.pw_last_error() and b'per-agent' in lib.pw_last_error(), lib.pw_last_error()
    _ring_untouched(mem, 'per-agent two-head ring')
    assert not buf.any()


def _refused(family, mem, match):
    from multiagent_rl_amd._lib import PworldError
    env, actor = _twin(family)
    before = _state(env)
    mem = _guard_ring(mem(env))
    rc = _raw_rollout(env, actor, mem)
    assert rc == -1 and env.last_kernel() == '', (rc, env.last_kernel())
    with pytest.raises(PworldError, match=match):
        actor.rollout(env, T, False, memory=mem)
    _ring_untouched(mem, family)
    assert actor.calls == CALLS0 and env.last_kernel() == ''
    for k, v in _state(env).items():
        _assert_same_bits(v, before[k], '%s: state.%s' % (family, k))


def test_the_rollout_sink_keeps_refusing_rings_of_another_kind():
    from multiagent_rl_amd.replay_buffer import ReplayBuffer
    cap = lambda env: T * env.num_envs + 5  # noqa: E731
    two = lambda env: ReplayBuffer(cap(env), env.n, env.obs_dim, act_heads=(5, 10), per_agent=True)  # noqa: E731
    # a two-head ring on simple_spread and on simple_tag (specialised and generic forms)
    for family in ('spread6-form3', 'spread14-auto', 'tag3+1-auto', 'spread6-form5'):
        _refused(family, two, 'two-head')
    # a single-head ring on simple_reference: through ctypes (FusedActor asserts the heads before the library sees the ring)
    env, actor = _twin('reference')
    mem = _guard_ring(ReplayBuffer(cap(env), env.n, env.obs_dim, per_agent=True))
    assert _raw_rollout(env, actor, mem) == -1 and b'two-head' in actor.lib.pw_last_error() and env.last_kernel() == ''
    _ring_untouched(mem, 'single-head ring on simple_reference')
    # a per-agent STATE ring on the generic form
    for family, desc in (('spread6-form5', FAMILIES['spread6-form3'][6]), ('tag3+1-form5', FAMILIES['tag3+1-auto'][6])):
        _refused(family, lambda env: ReplayBuffer(cap(env), env.n, env.obs_dim, per_agent=True, state_ring=desc), 'STATE ring')  # noqa: B023
    # a per-agent STATE ring of another scenario / shape
    tag_desc = dict(scenario='simple_tag', num_landmarks=2, num_adversaries=3)
    _refused('spread6-form3', lambda env: ReplayBuffer(cap(env), env.n, env.obs_dim, per_agent=True,
                                                       state_ring=dict(scenario='simple_spread', num_landmarks=5)), 'STATE ring')
    # (D = 16 is also a simple_tag row of six adversaries and one landmark: a consistent ring, of another scenario)
    _refused('spread6-form3', lambda env: ReplayBuffer(cap(env), env.n, env.obs_dim, per_agent=True,
                                                       state_ring=dict(scenario='simple_tag', num_landmarks=1, num_adversaries=6)),
             'another scenario')
    _refused('tag3+1-auto', lambda env: ReplayBuffer(cap(env), env.n, env.obs_dim, per_agent=True,
                                                     state_ring=dict(tag_desc, num_adversaries=2)), 'STATE ring')
    _refused('spread13-auto', lambda env: ReplayBuffer(cap(env), env.n + 1, env.obs_dim, per_agent=True), 'shape mismatch')


# ---- 8. the entry script


def test_the_bicnet_entry_trains_to_the_same_losses_on_its_state_ring_and_on_the_row_ring(tmp_path, monkeypatch):
    """examples/train_batched.py --critic bicnet --fused-targets at the size of tests/test_gpu_bicnet.py's entry test, once with the ring
    the script picks (the per-agent STATE ring) and once with --ring rows: same statistics (all but the wall time), same four losses."""
    sys.path.insert(0, os.path.join(ROOT, 'examples'))
    import madr_learner
    import train_batched as entry
    from multiagent_rl_amd import arglist
    runs = []
    inner = madr_learner.Trainer.optimize
    losses, seen = [], {}

    def recording(self):
        seen['memory'] = self.memory
        out = inner(self)
        losses.append(out)
        return out
    monkeypatch.setattr(madr_learner.Trainer, 'optimize', recording)
    saved = (arglist.num_episodes, arglist.save_rate, arglist.warmup_steps, arglist.batch_size)
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        arglist.warmup_steps, arglist.batch_size = 256, 256
        for ring in ('auto', 'rows'):
            del losses[:]
            res = entry.main(['--scenario', 'simple_spread', '--envs', '16', '--agents', '3', '--episodes', '64', '--chunk', '50',
                              '--save-rate', '32', '--max-updates-per-chunk', '2', '--out-dir', str(tmp_path / ring),
                              '--critic', 'bicnet', '--fused-targets', '--ring', ring])
            (name, cnt, st), = res
            runs.append((dict(st), [tuple(np.asarray(x, dtype=np.float64).ravel().tolist()) for x in losses], seen['memory']))
    finally:
        os.chdir(cwd)
        arglist.num_episodes, arglist.save_rate, arglist.warmup_steps, arglist.batch_size = saved
    (st_a, loss_a, mem_a), (st_b, loss_b, mem_b) = runs
    assert st_a['episodes'] == 64 and st_a['env_steps'] == 100 * 16 and st_a['updates'] == 4
    timing = ('wall_s',)       # the one entry that is a clock reading
    assert {k: v for k, v in st_a.items() if k not in timing} == {k: v for k, v in st_b.items() if k not in timing}
    assert len(loss_a) == len(loss_b) == 4 and np.isfinite(np.array(loss_a)).all()
    assert np.array_equal(np.array(loss_a).view(np.uint64), np.array(loss_b).view(np.uint64)), (loss_a, loss_b)
    assert mem_a.state_ring is not None and mem_b.state_ring is None
    for mem in (mem_a, mem_b):
        assert mem.per_agent is True and mem.rew.shape[1] == 3 and mem.done.shape[1] == 3 and len(mem) == st_a['env_steps']
