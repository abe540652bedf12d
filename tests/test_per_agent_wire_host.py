"""No GPU: the host side of the per-agent wire blocks (0.1.23).

(a) The library carries ``pw_wire_agent_rew_bytes`` and the three ``pw_replay_add_*wire_agents`` entry points, the header declares them
    and ``_lib.SIGNATURES`` binds them; the three block structs keep their bytes (held against the header's documented plane list, not
    against the library).
(b) Every ``*_agents`` entry point refuses, on the host and with a message that names it, what it does not serve.
(c) ``train_batched(per_agent_transition=True, gather=g)`` is served for a per-agent gather and for no other.
(d) A per-agent state gather at C2 ships 21 N + 5 bytes per env-step plus the per-chunk planes.
"""
import ctypes as C
import os
import re

import pytest
import torch

from multiagent_rl_amd import _lib
from multiagent_rl_amd.dist import FullTransitionGather

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('pw_wire_agent_rew_bytes', 'pw_replay_add_wire_agents', 'pw_replay_add_state_wire_agents', 'pw_replay_add_ref_wire_agents')


def test_the_version_was_raised_and_the_four_names_are_declared_and_bound():
    lib = _lib.load()
    assert lib.pw_version() >= 123
    header = open(os.path.join(ROOT, 'include', 'pworld.h')).read()
    assert int(re.search(r'#define\s+PW_VERSION\s+(\d+)', header).group(1)) >= 123
    for name in NAMES:
        assert re.search(r'\b(?:int|size_t)\s+%s\(' % name, header), name
        assert name in _lib.SIGNATURES and getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    for name in NAMES[1:]:          # (st, start, w, wire, rew_agents, stream)
        assert len(_lib.SIGNATURES[name][1]) == 6 and _lib.SIGNATURES[name][0] is C.c_int


def test_the_trailer_plane_is_sized_in_256_byte_steps():
    lib = _lib.load()
    assert lib.pw_wire_agent_rew_bytes(10, 8, 6) == 2048            # 1920 bytes of floats, rounded up
    for T, B, N in ((1, 1, 1), (10, 8, 6), (26, 37, 6), (15, 21, 3), (100, 4096, 6), (100, 8192, 6), (20, 33, 2), (7, 9, 64)):
        n = lib.pw_wire_agent_rew_bytes(T, B, N)
        assert n % 256 == 0 and 4 * T * B * N <= n < 4 * T * B * N + 256, (T, B, N, n)
    assert lib.pw_wire_agent_rew_bytes(0, 8, 6) == 0 and lib.pw_wire_agent_rew_bytes(10, 0, 6) == 0 and lib.pw_wire_agent_rew_bytes(10, 8, 0) == 0


def _planes(sizes):
    """Offsets of planes laid one behind the other, each on a 256-byte boundary, and the total (include/pworld.h: 'Planes, 256-B aligned')."""
    offs, off = [], 0
    for n in sizes:
        offs.append(off)
        off = (off + n + 255) // 256 * 256
    return offs, off


def _expect(struct, ints, sizes, tail=()):
    lay = struct()
    offs, total = _planes(sizes)
    names = [n for n, _ in struct._fields_]
    for name, v in zip(names, list(ints) + offs + [total] + list(tail)):
        setattr(lay, name, v)
    return lay


@pytest.mark.parametrize('T,B,ep', [(100, 4096, 25), (100, 8192, 25), (26, 37, 7)])
def test_the_three_block_structs_keep_their_bytes(T, B, ep):
    """The plane lists of include/pworld.h, restated: a per-agent block is the SAME block with a plane behind it."""
    lib = _lib.load()
    F = -(-T // ep)
    # pw_chunk_wire at C2 (N = 6, D = 16): obs0, obs, final_rows, rew_shared, act, fin_slot
    N, D = 6, 16
    got = _lib.PwChunkWire()
    assert lib.pw_chunk_wire_layout(T, B, N, D, ep, C.byref(got)) == 0
    want = _expect(_lib.PwChunkWire, (T, B, N, D, F, 0), (4 * B * N * D, 4 * T * B * N * D, 4 * F * B * N * D, 4 * T * B, T * B * N, T * B))
    assert bytes(got) == bytes(want)
    # pw_state_wire: state0, state, final_state, lm [(F+1),B,L] float2, ep0, rew_shared, act, epi -- C2 (L = 6) and simple_tag 4 + 2 (L = 2)
    for scen, L, A, Dd in ((_lib.PW_SIMPLE_SPREAD, 6, 0, 16), (_lib.PW_SIMPLE_TAG, 2, 4, 4 + 4 + 10 + 4)):
        got = _lib.PwStateWire()
        assert lib.pw_state_wire_layout_scn(scen, T, B, N, L, A, ep, C.byref(got)) == 0
        want = _expect(_lib.PwStateWire, (T, B, N, L, Dd, F),
                       (16 * B * N, 16 * T * B * N, 16 * F * B * N, 8 * (F + 1) * B * L, 4 * B, 4 * T * B, T * B * N, T * B), tail=(scen, A))
        assert bytes(got) == bytes(want), scen
    # pw_ref_wire: head0, head, final_head, goal, comm0, rew_shared, act [T,B,2,2], epi
    got = _lib.PwRefWire()
    assert lib.pw_ref_wire_layout(T, B, ep, C.byref(got)) == 0
    want = _expect(_lib.PwRefWire, (T, B, F, 0), (4 * B * 16, 4 * T * B * 16, 4 * F * B * 16, (F + 1) * B * 2, B * 2, 4 * T * B, T * B * 4, T * B))
    assert bytes(got) == bytes(want)


def _ring(N, D, per_agent=1, cap=1000, **kw):
    st = _lib.PwReplayStore()
    st.obs, st.next_obs, st.rew, st.done, st.act, st.lm = 4096, 8192, 12288, 16384, 20480, 24576      # fake, aligned "device pointers"
    st.capacity, st.num_agents, st.obs_dim, st.per_agent = cap, N, D, per_agent
    for k, v in kw.items():
        setattr(st, k, v)
    return st


def test_every_agents_entry_point_refuses_on_the_host_what_it_does_not_serve():
    """Nothing is launched (there is no GPU here): every refusal is PW_EINVAL with a message naming the entry point."""
    lib = _lib.load()
    wire, trailer = C.c_void_p(1 << 20), C.c_void_p(1 << 24)
    T, B = 10, 8

    def refused(rc, who, *words):
        msg = lib.pw_last_error()
        assert rc == -1 and who in msg and all(w in msg for w in words), (rc, msg)

    cw, sw, tw, rw = _lib.PwChunkWire(), _lib.PwStateWire(), _lib.PwStateWire(), _lib.PwRefWire()
    assert lib.pw_chunk_wire_layout(T, B, 6, 16, 25, C.byref(cw)) == 0
    assert lib.pw_state_wire_layout_scn(_lib.PW_SIMPLE_SPREAD, T, B, 6, 6, 0, 25, C.byref(sw)) == 0
    assert lib.pw_state_wire_layout_scn(_lib.PW_SIMPLE_TAG, T, B, 6, 2, 4, 25, C.byref(tw)) == 0
    assert lib.pw_ref_wire_layout(T, B, 25, C.byref(rw)) == 0
    two = dict(act_heads=2)
    calls = (
        # entry point, its block, a ring it would serve (keywords), a ring of another shape
        (lib.pw_replay_add_wire_agents, b'pw_replay_add_wire_agents', cw, (6, 16, {}), (5, 16, {})),
        (lib.pw_replay_add_state_wire_agents, b'pw_replay_add_state_wire_agents', sw, (6, 16, {}), (6, 14, {})),
        (lib.pw_replay_add_state_wire_agents, b'pw_replay_add_state_wire_agents', sw,
         (6, 16, dict(state_rows=1, num_landmarks=6, scenario=_lib.PW_SIMPLE_SPREAD)), (3, 16, dict(state_rows=1, num_landmarks=6))),
        (lib.pw_replay_add_ref_wire_agents, b'pw_replay_add_ref_wire_agents', rw, (2, 21, two), (3, 21, two)),
    )
    for fn, who, w, (N, D, kw), (N2, D2, kw2) in calls:
        def ring(n=N, d=D, k=kw, **more):
            st = _ring(n, d, **dict(k, **more))
            if st.act_heads == 2:
                st.head_width[0], st.head_width[1] = 5, 10
            return st
        refused(fn(C.byref(ring(per_agent=0)), 0, C.byref(w), wire, trailer, None), who, b'shared-reward', who[:-len('_agents')])   # a shared ring
        refused(fn(C.byref(ring()), 0, C.byref(w), wire, None, None), who, b'rew_agents')                                             # a null trailer
        refused(fn(C.byref(ring()), 0, C.byref(w), wire, C.c_void_p((1 << 24) + 2), None), who, b'rew_agents')                        # a misaligned one
        refused(fn(C.byref(ring(N2, D2, kw2)), 0, C.byref(w), wire, trailer, None), who, b'mismatch')                                  # another shape
        refused(fn(C.byref(ring(cap=T * B - 1)), 0, C.byref(w), wire, trailer, None), who, b'must fit the ring')                       # chunk > ring
    # a spread block into a tag STATE ring of the block's N and D ... (D = 16 = 4 + 2*2 + 2*(3 - 1) + 2*(3 - 1): a tag roster of the same width)
    sw3 = _lib.PwStateWire()
    assert lib.pw_state_wire_layout_scn(_lib.PW_SIMPLE_SPREAD, T, B, 3, 6, 0, 25, C.byref(sw3)) == 0 and sw3.D == 16
    tag = _ring(3, 16, state_rows=1, num_landmarks=2, scenario=_lib.PW_SIMPLE_TAG, num_adversaries=1)
    refused(lib.pw_replay_add_state_wire_agents(C.byref(tag), 0, C.byref(sw3), wire, trailer, None), b'pw_replay_add_state_wire_agents', b'scenario mismatch')
    # ... and into the tag 4 + 2 ring (another width)
    tag = _ring(6, 22, state_rows=1, num_landmarks=2, scenario=_lib.PW_SIMPLE_TAG, num_adversaries=4)
    refused(lib.pw_replay_add_state_wire_agents(C.byref(tag), 0, C.byref(sw), wire, trailer, None), b'pw_replay_add_state_wire_agents', b'mismatch')
    # a two-head ring for a single-head block and the reverse
    th = _ring(6, 16, act_heads=2)
    refused(lib.pw_replay_add_wire_agents(C.byref(th), 0, C.byref(cw), wire, trailer, None), b'pw_replay_add_wire_agents', b'two-head')
    refused(lib.pw_replay_add_state_wire_agents(C.byref(th), 0, C.byref(sw), wire, trailer, None), b'pw_replay_add_state_wire_agents', b'two-head')
    refused(lib.pw_replay_add_ref_wire_agents(C.byref(_ring(2, 21)), 0, C.byref(rw), wire, trailer, None), b'pw_replay_add_ref_wire_agents', b'two-head')
    # the plain entry points keep refusing the per-agent ring (tests/test_per_agent_sink_host.py holds their messages)
    assert lib.pw_replay_add_wire(C.byref(_ring(6, 16)), 0, C.byref(cw), wire, None) == -1 and b'per-agent' in lib.pw_last_error()


# ---- train_batched: which gather is served --------------------------------------------------------------------------------------
class _Args(object):
    max_episode_len, num_episodes, is_training = 25, 32, True
    batch_size, warmup_steps, update_rate, save_rate, display = 8, 1024, 100, 32, False


class _Memory(object):
    per_agent = True

    def __init__(self):
        self.n = 0

    def __len__(self):
        return self.n


class _Gather(object):
    """FullTransitionGather's surface as train_batched uses it."""

    def __init__(self, env, T, per_agent):
        self.per_agent, self.memory, self.T, self.env, self.calls = per_agent, _Memory(), T, env, 0

    def outputs(self):
        e = self.env
        return dict(obs=torch.zeros(self.T, e.num_envs, e.n, e.obs_dim), rew=-torch.ones(self.T, e.num_envs, e.n),
                    terminal=torch.zeros(self.T, e.num_envs, dtype=torch.bool))

    def __call__(self, obs0):
        self.calls += 1
        self.memory.n += self.T * self.env.num_envs

    def wait_ingested(self):
        pass

    def finish(self):
        pass


def test_train_batched_serves_a_per_agent_gather_and_no_other(tmp_path):
    from multiagent_rl_amd.train import train_batched
    from tests.test_train_entry import _StubEnv, _StubRollout, _StubTrainer
    trace, learners = [], []

    class _Trainer(_StubTrainer):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            learners.append(self)

    _StubTrainer.trace = trace

    class _Fused(object):
        def refresh(self):
            pass

        def rollout(self, env, T, out, stats=None):
            out['terminal'][T - 1] = True                  # every env finishes an episode per chunk
            stats[2].add_(env.num_envs)

    def make_rollout(env, actor, memory, seed):
        assert memory is None                              # with a gather the rollout has no ring of its own
        return _Fused(), _StubRollout(env, memory, trace)

    kw = dict(arglist=_Args(), out_dir=str(tmp_path), log=lambda *a: None, chunk=10, make_rollout=make_rollout)
    env = _StubEnv()
    g = _Gather(env, 10, per_agent=True)
    hist = train_batched(env, 'actor', 'critic', _Trainer, 'simple_spread', 'Discrete', per_agent_transition=True, gather=g, **kw)
    assert hist['stats']['episodes'] == 32 and g.calls == 2
    assert learners[-1].memory is g.memory                 # the gather's ring is the learner's
    with pytest.raises(ValueError, match='per_agent_transition=True with gather='):           # the old message, for every other gather
        train_batched(env, 'actor', 'critic', _Trainer, 'simple_spread', 'Discrete', per_agent_transition=True, gather=object(), **kw)
    with pytest.raises(ValueError, match='per_agent_transition=True with gather='):
        train_batched(env, 'actor', 'critic', _Trainer, 'simple_spread', 'Discrete', per_agent_transition=True,
                      gather=_Gather(env, 10, per_agent=False), **kw)
    with pytest.raises(ValueError, match='per-agent gather'):                                  # a per-agent gather for a shared-reward learner
        train_batched(env, 'actor', 'critic', _Trainer, 'simple_spread', 'Discrete', gather=_Gather(env, 10, per_agent=True), **kw)
    with pytest.raises(ValueError, match="per_agent_transition=True with ring='state'"):      # the STATE ring comes with the gather
        train_batched(env, 'actor', 'critic', _Trainer, 'simple_spread', 'Discrete', per_agent_transition=True, ring='state', gather=g, **kw)


# ---- the gather's own arithmetic, without a device ------------------------------------------------------------------------------
def _standin(per_agent, T=100, B=4096, N=6, L=6):
    g = FullTransitionGather.__new__(FullTransitionGather)
    g.T, g.B, g.N, g.L, g.D, g.A = T, B, N, L, 4 + 2 * L, 0
    g.scenario, g.max_episode_len, g.state_wire, g.ref_wire, g.per_agent = 'simple_spread', 25, True, False, per_agent
    g.lay = g._layout(_lib.PwStateWire)
    return g


def test_a_per_agent_state_gather_ships_21n_plus_5_bytes_per_env_step_at_c2():
    shared, agents = _standin(False), _standin(True)
    assert 113 < shared.bytes_per_env_step < 115                    # 17 N + 5 = 107, + (1 + F) state / landmark batches per chunk
    assert 137 < agents.bytes_per_env_step < 141                    # 114 + 24 plus padding
    assert agents.block_bytes - shared.block_bytes == _lib.load().pw_wire_agent_rew_bytes(100, 4096, 6) == 4 * 100 * 4096 * 6
    assert bytes(agents.lay) == bytes(shared.lay) and agents.lay.total_bytes % 256 == 0
    block = torch.zeros(agents.block_bytes, dtype=torch.uint8)
    v = agents.views(block)
    assert tuple(v['rew_agents'].shape) == (100, 4096, 6) and v['rew_agents'].dtype == torch.float32
    v['rew_agents'].fill_(1.0)
    assert not block[:agents.lay.total_bytes].any() and block[agents.lay.total_bytes:].view(torch.float32).eq(1.0).all()   # the trailer, nothing else
    assert 'rew_agents' not in shared.views(torch.zeros(shared.block_bytes, dtype=torch.uint8))


def test_a_ring_of_the_other_kind_is_refused_at_construction():
    class _Env(object):
        num_envs, n, obs_dim, num_landmarks, scenario_name, max_episode_len, local_observation = 8, 3, 10, 3, 'simple_spread', 25, True

    class _Ring(object):
        def __init__(self, per_agent):
            self.per_agent = per_agent

    with pytest.raises(ValueError, match='shared-reward ring'):
        FullTransitionGather(_Env(), 10, 0, 1, 'cpu', memory=_Ring(False), per_agent=True)
    with pytest.raises(ValueError, match='per-agent ring'):
        FullTransitionGather(_Env(), 10, 0, 1, 'cpu', memory=_Ring(True))
