"""GPU: the episode statistics (episode_return [B], finished_sum, finished_count -> mean_episode_reward) of all nine HIP producers
against an independent ledger (tests/episode_ledger_ref.py: run.py:55-65 restated in numpy, finished_sum by math.fsum).

Everywhere: episode_return bit for bit, finished_count exactly, |finished_sum - ledger| <= gamma_n * abs_sum (derived in the ledger's
docstring; nothing measured).  Every case starts from non-zero accumulators and runs at least two launches into them.

  producers 1-3 (pw_episode_stats / pw_rollout_tail, pw_replay_add_tail, pw_replay_add_rollout): synthetic inputs -- desynchronised
  ends, envs that finish nothing, envs that finish twice inside one launch (the second time on the last step), carry-in returns,
  rewards of both signs over seven decades; B on either side of 256 and 1024, T on either side of 8.
  producers 4-9 (the statistics sink of every one-launch policy rollout form): a small auto-resetting env with desynchronised episode
  clocks; the ledger is applied to the launch's own rew_shared / terminal outputs, and env.last_kernel() names the form that ran.
  one scratch, changing launch geometry: the sink's scratch must serve any sequence of forms on one handle (and two handles of equal
  (B, N) behind one FusedActor).
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

from tests import episode_ledger_ref as el  # noqa: E402

GENERIC = 'pw_policy_rollout_generic_kernel'


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _lib():
    from multiagent_rl_amd import _lib as m
    return m.load(), m.check


def _accumulators(ret0, sum0, count0):
    return (torch.from_numpy(np.array(ret0, np.float32)).cuda(), torch.tensor(float(sum0), dtype=torch.float64, device='cuda'),
            torch.tensor(int(count0), dtype=torch.int64, device='cuda'))


def _read(acc):
    return acc[0].cpu().numpy().copy(), float(acc[1].item()), int(acc[2].item())


def _clone(acc):
    return tuple(t.clone() for t in acc)


def _same_bits(a, b):
    ra, rb = _read(a), _read(b)
    return (np.array_equal(ra[0].view(np.uint32), rb[0].view(np.uint32)) and np.float64(ra[1]).view(np.uint64) == np.float64(rb[1]).view(np.uint64)
            and ra[2] == rb[2])


def _episode_stats(rew, term, acc):
    """pw_episode_stats: one step's rew_shared [B] / terminal [B] (device) into the accumulators."""
    lib, check = _lib()
    check(lib.pw_episode_stats(_p(rew), _p(term), rew.shape[0], _p(acc[0]), _p(acc[1]), _p(acc[2]), _stream()))


def _check_against_ledger(label, before, acc, rew, term):
    """``before`` = _read() of the accumulators ahead of the launch; rew / term = numpy [T,B] (or [B]) the launch consumed."""
    rew, term = np.asarray(rew, np.float32), np.asarray(term).astype(bool)
    if rew.ndim == 1:
        rew, term = rew[None], term[None]
    want = el.ledger(rew, term, before[0], before[1], before[2])
    got = _read(acc)
    el.check(got[0], got[1], got[2], want, label)
    return want


# ------------------------------------------------------------------------------------------
# producer 1: pw_episode_stats / pw_rollout_tail
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B', [1, 63, 1023, 1024, 1025, 3000])
def test_episode_stats_and_rollout_tail_against_the_ledger(B):
    """One workgroup of 1024 threads, env loop in strides of 1024, tree from 512 down: B = 1023 / 1024 / 1025 sit on either side of
    the stride, 3000 takes three trips.  Four launches into the same accumulators: two through pw_rollout_tail with BOTH device counters
    ((delta, modulo) = (B, cap), which wraps, and (1, 0), which never does), one with counter0 = NULL and counter1 set, one through
    pw_episode_stats (no counters).  The counters are checked against Python integers."""
    lib, check = _lib()
    case = el.synthetic_case(B, 1, calls=4, seed=1)
    acc = _accumulators(case['ret0'], case['sum0'], case['count0'])
    cap = B + B // 2 + 1
    c0, c1 = cap - 1, 2 ** 40 + 5                     # Python integers: what the device counters must hold
    d0 = torch.tensor(c0, dtype=torch.int64, device='cuda')
    d1 = torch.tensor(c1, dtype=torch.int64, device='cuda')
    wraps = 0
    for call in range(4):
        rew, term = torch.from_numpy(case['rew'][call, 0]).cuda(), torch.from_numpy(case['terminal'][call, 0]).cuda()
        before = _read(acc)
        if call < 2:
            check(lib.pw_rollout_tail(_p(rew), _p(term), B, _p(acc[0]), _p(acc[1]), _p(acc[2]), _p(d0), B, cap, _p(d1), 1, 0, _stream()))
            wraps += (c0 + B) >= cap
            c0, c1 = (c0 + B) % cap, c1 + 1
        elif call == 2:
            check(lib.pw_rollout_tail(_p(rew), _p(term), B, _p(acc[0]), _p(acc[1]), _p(acc[2]), None, 12345, 7, _p(d1), 3, 5, _stream()))
            c1 = (c1 + 3) % 5
        else:
            _episode_stats(rew, term, acc)
        _check_against_ledger('pw_rollout_tail B=%d call %d' % (B, call), before, acc, case['rew'][call, 0], case['terminal'][call, 0])
        assert int(d0.item()) == c0 and int(d1.item()) == c1, (call, int(d0.item()), c0, int(d1.item()), c1)
    assert wraps >= 1


# ------------------------------------------------------------------------------------------
# producer 2: pw_replay_add_tail
# ------------------------------------------------------------------------------------------
def _rows(B, T=None, seed=0):
    """Arbitrary ring rows for N = 1, D = 5."""
    g = torch.Generator().manual_seed(seed)
    shape = (B, 1, 5) if T is None else (T, B, 1, 5)
    return torch.randn(shape, generator=g).cuda(), torch.randint(0, 5, shape[:-1], generator=g, dtype=torch.int32).cuda()


@pytest.mark.parametrize('B', [1, 255, 256, 257, 1023, 1025, 2500])
def test_replay_add_tail_against_the_ledger_and_pw_episode_stats(B):
    """The bookkeeping workgroup of pw_replay_add_tail_kernel: 256 threads with four partial sums each (envs tid + 256 v + 1024 k).  Its
    comment claims pw_episode_stats' order, so beyond the ledger bound finished_sum must equal pw_episode_stats' on the same inputs BIT
    FOR BIT.  Three launches into the same accumulators: host cursor; device cursors (*next_start_dev == (start + B) % capacity across the
    ring's end, start_dev untouched, step_counter + 1); and terminal flags with final_obs = NULL, which still count."""
    from multiagent_rl_amd.replay_buffer import ReplayBuffer
    case = el.synthetic_case(B, 1, calls=3, seed=2)
    cap = 2 * B + 3
    mem = ReplayBuffer(cap, 1, 5)
    first = mem._next_idx = cap - B - (B + 1) // 2    # the second launch (device cursors) crosses the ring's end
    acc = _accumulators(case['ret0'], case['sum0'], case['count0'])
    step_counter = torch.tensor(77, dtype=torch.int64, device='cuda')
    for call in range(3):
        rew_np, term_np = case['rew'][call, 0], case['terminal'][call, 0]
        rew, term = torch.from_numpy(rew_np).cuda(), torch.from_numpy(term_np).cuda()
        obs, act = _rows(B, seed=10 * call)
        nxt, _ = _rows(B, seed=10 * call + 1)
        fin, _ = _rows(B, seed=10 * call + 2)
        before = _read(acc)
        twin = _clone(acc)
        _episode_stats(rew, term, twin)
        start = mem._next_idx
        if call == 0:
            mem.add_batch_tail(obs, act, rew, nxt, fin, term, *acc)
        elif call == 1:
            mem.sync_cursor()                         # both cells = the host position
            mem._cursor[1] = -1
            mem.add_batch_tail(obs, act, rew, nxt, fin, term, *acc, step_counter=step_counter, parity=0)
            assert start + B >= cap and mem._cursor.tolist() == [start, (start + B) % cap] and int(step_counter.item()) == 78
            mem.note_graph_adds(B)
        else:
            mem.add_batch_tail(obs, act, rew, nxt, None, term, *acc)
            assert int(step_counter.item()) == 78
        _check_against_ledger('pw_replay_add_tail B=%d call %d' % (B, call), before, acc, rew_np, term_np)
        assert _same_bits(acc, twin), 'pw_replay_add_tail and pw_episode_stats differ on the same inputs (call %d)' % call
        slots = (start + torch.arange(B, device='cuda')) % cap
        assert torch.equal(mem.rew[slots], rew) and torch.equal(mem.obs[slots], obs)
        want_next = torch.where(term[:, None, None], fin, nxt) if call < 2 else nxt
        assert torch.equal(mem.next_obs[slots], want_next)
    assert mem._next_idx == (first + 3 * B) % cap


# ------------------------------------------------------------------------------------------
# producer 3: pw_replay_add_rollout
# ------------------------------------------------------------------------------------------
def _chunk(case, call, T, B):
    obs, act = _rows(B, T, seed=100 + call)
    fin, _ = _rows(B, T, seed=200 + call)
    return dict(obs=obs, final_obs=fin, act=act, rew_shared=torch.from_numpy(case['rew'][call]).cuda(),
                terminal=torch.from_numpy(case['terminal'][call]).cuda())


@pytest.mark.parametrize('B,T', [(1, 1), (255, 7), (256, 8), (257, 9), (600, 17), (300, 31)])
def test_add_rollout_against_the_ledger(B, T):
    """The stat blocks of pw_replay_add_rollout_kernel: thread = env, T steps walked 8 at a time with a clamped tail (T = 7 / 8 / 9: one
    short trip, one full, one full + a tail of 1; 17 and 31: tails of 1 and 7; the generator ends an episode on the last step), one partial
    per 256 envs (B = 255 / 256 / 257: one full-minus-one block, one full, two; 600: three), a ticket picks the last block.  Two chunks
    with bookkeeping into the same accumulators and the same scratch, a chunk WITHOUT bookkeeping between them (accumulators and scratch
    untouched); episode_return bit-equal to T launches of pw_episode_stats; and the whole sequence again from equal state: identical
    bits in all three outputs."""
    from multiagent_rl_amd.replay_buffer import ReplayBuffer
    case = el.synthetic_case(B, T, calls=2, seed=3)
    mem = ReplayBuffer(2 * T * B + 5, 1, 5)           # five chunks below: the ring wraps
    obs0, _ = _rows(B, seed=5)
    chunks = [_chunk(case, c, T, B) for c in range(2)]
    results = []
    for run in range(2):
        acc = _accumulators(case['ret0'], case['sum0'], case['count0'])
        twin = _clone(acc)
        after = []
        for call in range(2):
            before = _read(acc)
            mem.add_rollout(obs0, chunks[call], *acc)
            _check_against_ledger('add_rollout B=%d T=%d run %d call %d' % (B, T, run, call), before, acc, case['rew'][call],
                                  case['terminal'][call])
            for t in range(T):
                _episode_stats(chunks[call]['rew_shared'][t], chunks[call]['terminal'][t], twin)
            assert torch.equal(acc[0].view(torch.int32), twin[0].view(torch.int32)), 'episode_return differs from T x pw_episode_stats'
            assert int(acc[2].item()) == int(twin[2].item())
            after.append(_clone(acc))
            if call == 0 and run == 0:                # a chunk without bookkeeping leaves the accumulators and the scratch alone
                scratch = mem._roll_scratch.clone()
                mem.add_rollout(obs0, chunks[1])
                assert _same_bits(acc, after[0]) and torch.equal(mem._roll_scratch, scratch)
        results.append(after)
    for call in range(2):
        assert _same_bits(results[0][call], results[1][call]), 'two runs from equal state differ (call %d)' % call


# ------------------------------------------------------------------------------------------
# producers 4-9: the statistics sink of the one-launch policy rollouts
# ------------------------------------------------------------------------------------------
MAX_LEN = 7


def _make_env(scenario, B, max_episode_len=MAX_LEN, form=0, **kw):
    from multiagent_rl_amd import make_batched_env
    env = make_batched_env(scenario, B, auto_reset=True, max_episode_len=max_episode_len, seed=21, **kw)
    if form:
        env.set_dispatch(policy_form=form)
    env.reset()
    st = env.get_state()
    ep0 = (np.arange(B) % max_episode_len).astype(np.int32)     # every env at another point of its episode
    env.set_state(st['pos'], st['vel'], st['landmarks'], ep_step=ep0, ep_count=st['ep_count'])
    return env, ep0


def _make_actor(env, seed=9):
    from multiagent_rl_amd.policy import ActorNetwork, FusedActor
    torch.manual_seed(4)
    heads = [5, env.dim_c] if env.scenario_name == 'simple_reference' else 5
    return FusedActor(ActorNetwork(env.obs_dim, heads).cuda().eval(), seed=seed)


def _carry_in(B):
    rng = np.random.RandomState(B)
    return _accumulators((rng.uniform(-3, 3, B) + 0.125).astype(np.float32), -12.5, 7)


def _launch_and_check(label, actor, env, T, acc, ep0, kernel, max_episode_len=MAX_LEN):
    """One FusedActor.rollout with step outputs and the statistics sink; the ledger on the launch's own outputs.  -> the clocks after."""
    before = _read(acc)
    out = actor.rollout(env, T, stats=acc)
    assert env.last_kernel() == kernel, (label, env.last_kernel())
    term = out['terminal'].cpu().numpy().astype(bool)
    assert np.array_equal(term, el.clock_terminals(ep0, T, max_episode_len)), label + ': the episode clocks are not where set_state put them'
    want = _check_against_ledger(label + ' ' + env.last_kernel(), before, acc, out['rew_shared'].cpu().numpy(), term)
    assert want['finished_count'] - before[2] == int(term.sum()) > 0
    return ((ep0 + T) % max_episode_len).astype(np.int32)


# id -> (scenario, kwargs, policy_form, B, T, kernel)
ROLLOUT_FORMS = {
    # 16 envs per workgroup: 3 workgroups, the last with 5 envs (ragged: envs_here < E)
    'v3-N3-ragged': ('simple_spread', dict(n=3), 0, 37, 20, 'pw_policy_rollout3_kernel'),
    # the N = 6, L = 6 instantiation; B < E: one workgroup with 5 of its 16 envs
    'v3-N6L6-B<E': ('simple_spread', dict(n=6), 0, 5, 20, 'pw_policy_rollout3_kernel'),
    'v3j-full-head': ('simple_spread', dict(n=16), 4, 37, 20, 'pw_policy_rollout3j_kernel'),
    # rows of 66 numbers: the half-storage head (the only form that serves them); T = 16 keeps the case short, two or three ends per env
    'v3j-half-head': ('simple_spread', dict(n=31), 0, 17, 16, 'pw_policy_rollout3j_kernel'),
    'tag-3+1': ('simple_tag', dict(num_adversaries=3, num_good=1), 0, 37, 20, 'pw_policy_rollout_tag_kernel'),
    'reference': ('simple_reference', dict(), 0, 17, 20, 'pw_policy_rollout_ref_kernel<3>'),
    'generic-full-obs': ('simple_spread', dict(n=3, local_observation=False), 0, 37, 20, GENERIC),
    # at most 96 rows per workgroup: 6 envs of 16 agents, 8 workgroups (multi-block ticket)
    'generic-N16-8wg': ('simple_spread', dict(n=16), 5, 48, 20, GENERIC),
}


@pytest.mark.parametrize('case', sorted(ROLLOUT_FORMS))
def test_rollout_sink_statistics_against_the_ledger(case):
    """Per env in registers, per workgroup through rollout_finish_stats (envs_here partials, a ticket, the last workgroup sums the
    partials): every kernel that carries the sink, on desynchronised clocks (max_episode_len = 7: every env ends two or three times per
    launch, on every step some env), non-zero carry-in, two launches, the second continuing from the first."""
    scenario, kw, form, B, T, kernel = ROLLOUT_FORMS[case]
    env, ep0 = _make_env(scenario, B, form=form, **kw)
    actor = _make_actor(env)
    acc = _carry_in(B)
    for launch in range(2):
        ep0 = _launch_and_check('%s launch %d' % (case, launch), actor, env, T, acc, ep0, kernel)


def test_rollout_sink_statistics_with_more_than_512_workgroups():
    """The multi-round branch of rollout_finish_stats: the last workgroup adds the partials up 512 per round.  The generic form with
    N = 16 holds 6 envs per workgroup: B = 3200 -> 534 workgroups, two rounds (the second with 22 partials)."""
    lib, _ = _lib()
    B, T, L = 3200, 8, 3
    env, ep0 = _make_env('simple_spread', B, max_episode_len=L, form=5, n=16)
    E = lib.pw_policy_generic_envs_per_workgroup(env.cfg.scenario, env.cfg.obs_mode, 16, 16, 0)
    assert 0 < E and (B + E - 1) // E > 512, E
    actor = _make_actor(env)
    acc = _carry_in(B)
    for launch in range(2):
        ep0 = _launch_and_check('generic %d workgroups launch %d' % ((B + E - 1) // E, launch), actor, env, T, acc, ep0, GENERIC,
                                max_episode_len=L)


# ------------------------------------------------------------------------------------------
# one scratch, changing launch geometry
# ------------------------------------------------------------------------------------------
def _generic_grid(env):
    lib, _ = _lib()
    E = lib.pw_policy_generic_envs_per_workgroup(env.cfg.scenario, env.cfg.obs_mode, env.n, env.num_landmarks, 0)
    assert E > 0
    return (env.num_envs + E - 1) // E


def test_one_scratch_serves_launches_of_different_geometry():
    """pworld.h: scratch of pw_policy_rollout_scratch_bytes(h) bytes, zeroed once, serves the handle -- whatever form a launch takes.
    simple_spread N = L = 16, B = 48, ONE FusedActor (one scratch tensor): policy_form 5 (generic: 6 envs per workgroup, grid 8), then
    policy_form 0 (just in time: the dispatcher takes that form only with >= 8 envs per workgroup -- 16 here -- so grid 3, at most 6),
    then policy_form 5 again.  Until 0.1.13 the ticket word sat BEHIND the partials, at word 2 * grid: the second launch's ticket
    (word 6) was the first launch's partial sum of workgroup 6, no workgroup drew the last ticket and the launch's finished episodes
    were dropped -- after the second launch: expected finished_count 7 + 137 + 137 = 281, observed 144 (episode_return was still right)."""
    B, T = 48, 20
    env, ep0 = _make_env('simple_spread', B, n=16)
    assert _generic_grid(env) == 8 and (B + 7) // 8 < 8      # any specialised launch the dispatcher accepts has fewer workgroups
    actor = _make_actor(env)
    acc = _carry_in(B)
    for launch, (form, kernel) in enumerate([(5, GENERIC), (0, 'pw_policy_rollout3j_kernel'), (5, GENERIC)]):
        env.set_dispatch(policy_form=form)
        ep0 = _launch_and_check('form %d (launch %d)' % (form, launch), actor, env, T, acc, ep0, kernel)
    assert actor._sink_scratch_key == (B, 16)


@pytest.mark.parametrize('N', [6, 16])
def test_one_actor_serves_two_envs_of_equal_shape_and_different_form(N):
    """FusedActor keeps one scratch per (B, N): two handles of equal shape, one under automatic dispatch (N = 6: pw_policy_rollout3_kernel,
    16 envs per workgroup; N = 16: the just-in-time form, 16) and one under policy_form 5 (the generic form: 16 and 6 envs per workgroup),
    take turns on it.  B = 40: grids 3 / 3 at N = 6, 3 / 7 at N = 16."""
    B, T = 40, 20
    env_a, ep_a = _make_env('simple_spread', B, n=N)
    env_g, ep_g = _make_env('simple_spread', B, form=5, n=N)
    auto = 'pw_policy_rollout3_kernel' if N == 6 else 'pw_policy_rollout3j_kernel'
    print('N = %d: generic grid %d, specialised grid %d' % (N, _generic_grid(env_g), (B + 15) // 16))
    actor = _make_actor(env_a)
    acc_a, acc_g = _carry_in(B), _carry_in(B)
    scratch = None
    for turn in range(2):
        ep_g = _launch_and_check('N=%d generic turn %d' % (N, turn), actor, env_g, T, acc_g, ep_g, GENERIC)
        ep_a = _launch_and_check('N=%d automatic turn %d' % (N, turn), actor, env_a, T, acc_a, ep_a, auto)
        assert scratch is None or scratch == actor._sink_scratch.data_ptr()
        scratch = actor._sink_scratch.data_ptr()


def test_stats_without_a_finished_episode_report_nan_and_zero_episodes():
    """BatchedRollout.stats() before any episode ended (T < max_episode_len): mean_episode_reward is nan, episodes 0 -- and the sink ran
    (the running returns moved)."""
    import math
    from multiagent_rl_amd import make_batched_env
    from multiagent_rl_amd.rollout import BatchedRollout
    env = make_batched_env('simple_spread', 37, n=3, auto_reset=True, max_episode_len=25, seed=21)
    ro = BatchedRollout(env, _make_actor(env), None)
    ro.collect_one_launch(3, chunk=3, keep_outputs=True)
    st = ro.stats()
    assert st['episodes'] == 0 and st['env_steps'] == 3 * 37 and math.isnan(st['mean_episode_reward'])
    assert not ro.last_chunk['terminal'].any()
    before = (np.zeros(37, np.float32), 0.0, 0)
    _check_against_ledger('no finished episode', before, (ro.episode_return, ro.finished_return_sum, ro.finished_episodes),
                          ro.last_chunk['rew_shared'].cpu().numpy(), ro.last_chunk['terminal'].cpu().numpy())
    assert (ro.episode_return != 0).all()
