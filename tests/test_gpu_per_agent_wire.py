"""GPU, one process: per-agent wire blocks (0.1.23) -- ``FullTransitionGather(world=1, per_agent=True)`` beside a twin env whose rollout
sink fills a per-agent ring of the same kind.  The sink is the existing, oracle-checked path (tests/test_gpu_per_agent_sink.py) and is
the reference here: after three chunks ``sample_index(range(n))`` of both rings is bit-identical in all five outputs.

The cases are the smallest that reach each append kernel's per-agent form and each way it can go wrong: N * D a multiple of four and not
(pw_replay_add_wire_agents_kernel<4> / <1>), an even and an odd number of landmarks (pw_replay_add_state_wire_agents_kernel<4> / <2>),
the units kernel (simple_tag into a row ring), the STATE ring of both scenarios, simple_reference's two-head ring; several workgroups
(a chunk is 9 000 to 70 000 threads), odd B and T, several episode ends per env inside a chunk (F >= 2), and a ring of 2 T B + 5 slots
under three chunks, so that the third chunk's slots wrap the ring's end.  The ring's planes sit in guarded buffers (tests/guarded.py).

Each case also holds that the TWIN's ring carries rewards that differ between the agents of one transition: the test cannot pass on a
broadcast of the shared reward.
"""
import ctypes as C
import functools

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

from tests.guarded import assert_guards_intact, guarded  # noqa: E402

CASES = {
    # name: scenario, env keywords, B, T, episode length, wire, ring, the kernel the root's append launches
    'spread6-row-blocks': ('simple_spread', dict(n=6), 37, 26, 7, 'rows', 'rows', 'pw_replay_add_wire_agents_kernel<4>'),
    'spread3-row-blocks': ('simple_spread', dict(n=3), 21, 15, 4, 'rows', 'rows', 'pw_replay_add_wire_agents_kernel<1>'),      # N D = 30
    'spread6-state-rows': ('simple_spread', dict(n=6), 37, 26, 7, 'state', 'rows', 'pw_replay_add_state_wire_agents_kernel<4>'),
    'spread3-state-rows': ('simple_spread', dict(n=3), 21, 15, 4, 'state', 'rows', 'pw_replay_add_state_wire_agents_kernel<2>'),  # odd L
    'spread6-state-ring': ('simple_spread', dict(n=6), 37, 26, 7, 'state', 'state', 'pw_replay_add_state_wire_to_state_ring_agents_kernel'),
    'tag2+3-rows': ('simple_tag', dict(num_adversaries=2, num_good=3), 37, 30, 11, 'state', 'rows', 'pw_replay_add_state_wire_units_agents_kernel'),
    'tag4+2-state-ring': ('simple_tag', dict(num_adversaries=4, num_good=2), 37, 30, 11, 'state', 'state',
                          'pw_replay_add_state_wire_to_state_ring_agents_kernel'),
    'reference': ('simple_reference', dict(), 33, 20, 6, 'auto', 'rows', 'pw_replay_add_ref_wire_agents_kernel'),
}
CHUNKS = 3
PLANES = ('obs', 'next_obs', 'act', 'rew', 'done', 'lm')


def _ring_kw(env, scenario, ring):
    if scenario == 'simple_reference':
        return dict(act_heads=(5, 10))
    if ring == 'state':
        return dict(state_ring=dict(scenario=scenario, num_landmarks=env.num_landmarks,
                                    num_adversaries=env.cfg.num_adversaries if scenario == 'simple_tag' else 0))
    return {}


def _guard_ring(mem):
    """Move the ring's planes into guarded buffers and point the store at them."""
    for k in PLANES:
        plane = getattr(mem, k, None)
        if plane is None:
            continue
        g = guarded(plane.shape, plane.dtype)
        setattr(mem, k, g)
        setattr(mem._store, k, g.data_ptr())
    return mem


@functools.lru_cache(maxsize=None)
def _run(case):
    from multiagent_rl_amd import make_batched_env
    from multiagent_rl_amd.dist import FullTransitionGather
    from multiagent_rl_amd.policy import ActorNetwork, FusedActor
    from multiagent_rl_amd.replay_buffer import ReplayBuffer
    scenario, kw, B, T, ep, wire, ring, _ = CASES[case]
    dev = torch.device('cuda', 0)
    torch.manual_seed(0)
    mk = lambda: make_batched_env(scenario, B, auto_reset=True, max_episode_len=ep, seed=11, env_id_base=5, **kw)  # noqa: E731
    env_a, env_b = mk(), mk()
    N, D = env_a.n, env_a.obs_dim
    net = ActorNetwork(D, [5, 10] if scenario == 'simple_reference' else 5).to(dev).eval()
    wire_actor, sink_actor = FusedActor(net, seed=3), FusedActor(net, seed=3)
    cap = 2 * T * B + 5
    rkw = _ring_kw(env_a, scenario, ring)
    mem = _guard_ring(ReplayBuffer(cap, N, D, per_agent=True, device_index=True, **rkw))
    full = FullTransitionGather(env_a, T, 0, 1, dev, memory=mem, wire=wire, ring=ring, per_agent=True)
    assert full.per_agent and full.memory is mem and full.lay.F >= 2 and full.side['rew'] is None
    assert all(w.numel() == full.lay.total_bytes + 256 * -(-4 * T * B * N // 256) for w in full.wire)
    want = ReplayBuffer(cap, N, D, per_agent=True, **rkw)
    env_a.reset()
    env_b.reset()
    obs0 = env_a.observe()
    rews = []
    for k in range(CHUNKS):
        out = full.outputs()
        assert out['rew'].data_ptr() == full.wire[k % 3].data_ptr() + full.lay.total_bytes      # a view into the block's trailer
        wire_actor.rollout(env_a, T, out)
        rews.append(out['rew'].clone())
        full(obs0)
        obs0 = out['obs'][T - 1].clone()
        sink_actor.rollout(env_b, T, False, memory=want)
    full.finish()
    torch.cuda.synchronize()
    assert full.rows_ingested == CHUNKS * T * B and len(mem) == len(want) == cap and mem._next_idx == want._next_idx == (CHUNKS * T * B) % cap
    return dict(mem=mem, want=want, full=full, rew=torch.cat(rews).reshape(CHUNKS * T * B, N), cap=cap, N=N, D=D, T=T, B=B)


@pytest.mark.parametrize('case', sorted(CASES))
def test_the_gathered_per_agent_ring_is_the_twin_sinks_ring_bit_for_bit(case):
    r = _run(case)
    mem, want, cap, N, D = r['mem'], r['want'], r['cap'], r['N'], r['D']
    scenario, ring = CASES[case][0], CASES[case][6]
    idx = list(range(cap))
    got_b, want_b = mem.sample_index(idx), want.sample_index(idx)
    # a condition on the INPUTS: the twin's rewards differ between the agents of a transition (this is no broadcast of rew_shared)
    w_rew = want_b[2]
    assert tuple(w_rew.shape) == (cap, N)
    assert int((w_rew.max(1).values != w_rew.min(1).values).sum()) >= 1, 'the twin ring holds one reward per transition: choose another seed'
    for name, g, w in zip(('obs', 'act', 'rew', 'next_obs', 'done'), got_b, want_b):
        assert g.shape == w.shape and g.dtype == w.dtype, name
        assert torch.equal(g.view(torch.int32), w.view(torch.int32)), '%s: sample_index %s differs from the twin sink ring' % (case, name)
    assert tuple(got_b[0].shape) == (cap, N, D) and tuple(got_b[4].shape) == (cap, N)
    assert tuple(mem.done.shape) == (cap, N) and not mem.done.any() and not got_b[4].any()
    # the planes themselves, where the two rings keep the same thing (every slot was written: three chunks into 2 T B + 5 slots)
    for k in PLANES:
        if getattr(mem, k, None) is not None:
            assert torch.equal(getattr(mem, k), getattr(want, k)), '%s: ring.%s' % (case, k)
            assert_guards_intact(getattr(mem, k), '%s: ring.%s' % (case, k))
    assert (mem.state_ring is not None) == (ring == 'state') and tuple(mem.obs.shape[1:]) == ((N, 4) if ring == 'state' else (N, D))
    # the ring's rew plane is what the rollout wrote into the trailers, in slot order (the third chunk wraps)
    T, B = r['T'], r['B']
    slots = torch.arange(CHUNKS * T * B, device='cuda') % cap
    last = {int(s): i for i, s in enumerate(slots.tolist())}          # a slot written twice keeps the later transition
    keep = torch.tensor(sorted(last.values()), device='cuda')
    assert torch.equal(mem.rew[slots[keep]], r['rew'][keep])
    assert (scenario == 'simple_reference') == (mem.act.dim() == 3)


def _sentinel(plane):
    return (torch.arange(plane.numel(), device=plane.device) % 251).reshape(plane.shape).to(plane.dtype)


def _untouched(mem, what):
    torch.cuda.synchronize()
    for k in PLANES:
        plane = getattr(mem, k, None)
        if plane is not None:
            assert_guards_intact(plane, '%s: ring.%s' % (what, k))
            assert torch.equal(plane, _sentinel(plane)), '%s: ring.%s was written' % (what, k)


def test_the_agents_entry_points_refuse_a_shared_ring_and_a_null_trailer_on_the_device():
    """Each ``*_agents`` call on a shared ring, and on a null trailer, returns -1, leaves a sentinel-filled ring (guarded) untouched and
    launches nothing; the inputs it is handed are never read (a zero buffer stands in for all of them)."""
    from multiagent_rl_amd import _lib
    from multiagent_rl_amd.replay_buffer import ReplayBuffer
    lib = _lib.load()
    T, B, N, L, D = 7, 9, 6, 6, 16
    buf = torch.zeros(1 << 20, dtype=torch.uint8, device='cuda')
    p = C.c_void_p(buf.data_ptr())
    trailer = C.c_void_p(buf.data_ptr() + (1 << 19))
    cw, sw, rw = _lib.PwChunkWire(), _lib.PwStateWire(), _lib.PwRefWire()
    assert lib.pw_chunk_wire_layout(T, B, N, D, 3, C.byref(cw)) == 0 and cw.total_bytes <= 1 << 19
    assert lib.pw_state_wire_layout_scn(_lib.PW_SIMPLE_SPREAD, T, B, N, L, 0, 3, C.byref(sw)) == 0 and sw.total_bytes <= 1 << 19
    assert lib.pw_ref_wire_layout(T, B, 3, C.byref(rw)) == 0 and rw.total_bytes <= 1 << 19
    state = dict(state_ring=dict(scenario='simple_spread', num_landmarks=L))
    calls = (('pw_replay_add_wire_agents', cw, (N, D, {})), ('pw_replay_add_state_wire_agents', sw, (N, D, {})),
             ('pw_replay_add_state_wire_agents', sw, (N, D, state)), ('pw_replay_add_ref_wire_agents', rw, (2, 21, dict(act_heads=(5, 10)))))
    for name, w, (n, d, kw) in calls:
        fn = getattr(lib, name)
        for per_agent, tr, word in ((False, trailer, b'shared-reward'), (True, None, b'rew_agents')):
            mem = _guard_ring(ReplayBuffer(T * B + 5, n, d, per_agent=per_agent, **kw))
            for k in PLANES:
                if getattr(mem, k, None) is not None:
                    getattr(mem, k).copy_(_sentinel(getattr(mem, k)))
            rc = fn(C.byref(mem._store), 0, C.byref(w), p, tr, _lib.stream(torch.device('cuda', 0)))
            msg = lib.pw_last_error()
            assert rc == -1 and name.encode() in msg and word in msg, (name, per_agent, rc, msg)
            _untouched(mem, '%s, per_agent=%s' % (name, per_agent))
    assert not buf.any()
