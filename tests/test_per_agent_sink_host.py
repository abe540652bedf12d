"""No GPU: the host side of the per-agent ring sink (0.1.22).

(a) ``BatchedRollout.collect_one_launch`` with a per-agent memory hands the ring to ``policy.rollout`` -- one call per chunk -- and never
    calls ``memory.add_rollout`` (until 0.1.21 it ran the rollout with the statistics sink alone and appended with a second launch);
    ``keep_outputs`` keeps its meaning.
(b) The library's version was raised, and the tail / packed / wire entry points refuse a per-agent ring on the host, before anything
    could be launched, with a message that names the reason.
"""
import ctypes as C
import os
import re

import pytest
import torch

from multiagent_rl_amd import _lib
from multiagent_rl_amd.rollout import BatchedRollout
from tests.test_train_entry import _StubEnv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Cfg(object):
    auto_reset = True


class _Env(_StubEnv):
    cfg = _Cfg()

    def reset(self):
        return torch.zeros(self.num_envs, self.n, self.obs_dim)

    observe = reset


class _PerAgentRing(object):
    per_agent = True

    def __init__(self):
        self.appended = 0

    def add_rollout(self, *a, **k):
        raise AssertionError('collect_one_launch appended with a second launch (memory.add_rollout)')

    add_batch = add_rollout


class _Policy(object):
    """FusedActor.rollout's surface: records its calls, 'appends' the chunk to the ring it was given."""

    def __init__(self):
        self.calls = []

    def rollout(self, env, num_steps, out=None, memory=None, stats=None):
        self.calls.append(dict(T=num_steps, out=out, memory=memory, stats=stats))
        memory.appended += num_steps * env.num_envs
        return dict(rew=torch.zeros(num_steps, env.num_envs, env.n)) if out is not False else {}


@pytest.mark.parametrize('keep_outputs', [False, True])
def test_collect_one_launch_hands_a_per_agent_ring_to_the_rollouts_sink(keep_outputs):
    env, mem, pol = _Env(), _PerAgentRing(), _Policy()
    ro = BatchedRollout(env, pol, mem)
    assert ro._per_agent_memory()
    assert ro.collect_one_launch(12, chunk=5, keep_outputs=keep_outputs) == 12 * env.num_envs
    assert [c['T'] for c in pol.calls] == [5, 5, 2]                      # one call per chunk
    assert all(c['memory'] is mem for c in pol.calls) and mem.appended == 12 * env.num_envs
    for c in pol.calls:
        assert len(c['stats']) == 3 and c['stats'][0] is ro.episode_return
        assert (c['out'] is not False) == keep_outputs
    if keep_outputs:
        assert tuple(ro.last_chunk['rew'].shape) == (2, env.num_envs, env.n)
    assert not hasattr(ro, '_pa_chunks')


def test_the_version_was_raised_and_the_header_says_what_is_served():
    lib = _lib.load()
    assert lib.pw_version() >= 122
    header = open(os.path.join(ROOT, 'include', 'pworld.h')).read()
    assert int(re.search(r'#define\s+PW_VERSION\s+(\d+)', header).group(1)) >= 122
    assert '0.1.22' in header and 'take the plain ring only' not in header


def test_the_tail_packed_and_wire_entry_points_refuse_a_per_agent_ring_on_the_host():
    lib = _lib.load()
    st = _lib.PwReplayStore()
    st.obs, st.next_obs, st.rew, st.done, st.act, st.lm = 4096, 8192, 12288, 16384, 20480, 24576      # fake, aligned "device pointers"
    st.capacity, st.num_agents, st.obs_dim, st.per_agent = 1000, 6, 16, 1
    p = C.c_void_p(4096)
    wire = C.c_void_p(1 << 20)
    T, B = 10, 8

    def refused(rc, who):
        msg = lib.pw_last_error()
        assert rc == -1 and who in msg and b'per-agent' in msg, (rc, msg)

    for state_rows in (0, 1):
        st.state_rows, st.num_landmarks, st.scenario = state_rows, 6 * state_rows, _lib.PW_SIMPLE_SPREAD
        refused(lib.pw_replay_add_tail(C.byref(st), 0, None, None, B, p, p, p, p, p, p, None, p, p, p, None, None), b'pw_replay_add_tail')
        refused(lib.pw_replay_add_packed(C.byref(st), 0, 4, p, None), b'pw_replay_add_packed')
        cw = _lib.PwChunkWire()
        assert lib.pw_chunk_wire_layout(T, B, 6, 16, 25, C.byref(cw)) == 0
        refused(lib.pw_replay_add_wire(C.byref(st), 0, C.byref(cw), wire, None), b'pw_replay_add_wire')
        sw = _lib.PwStateWire()
        assert lib.pw_state_wire_layout_scn(_lib.PW_SIMPLE_SPREAD, T, B, 6, 6, 0, 25, C.byref(sw)) == 0
        refused(lib.pw_replay_add_state_wire(C.byref(st), 0, C.byref(sw), wire, None), b'pw_replay_add_state_wire')
    two = _lib.PwReplayStore()
    two.obs, two.next_obs, two.rew, two.done, two.act = 4096, 8192, 12288, 16384, 20480
    two.capacity, two.num_agents, two.obs_dim, two.per_agent, two.act_heads = 1000, 2, 21, 1, 2
    two.head_width[0], two.head_width[1] = 5, 10
    rw = _lib.PwRefWire()
    assert lib.pw_ref_wire_layout(T, B, 25, C.byref(rw)) == 0
    refused(lib.pw_replay_add_ref_wire(C.byref(two), 0, C.byref(rw), wire, None), b'pw_replay_add_ref_wire')
