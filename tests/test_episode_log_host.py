"""CPU: the episode log without a GPU -- its reference model (tests/episode_log_ref.py) against the two host ledgers the project has, the
chronological merge of per-rank histories, the control flow of ``train.evaluate_batched`` and ``train_batched(ledger='device')`` with
stubs and the model in the log's place, and what ``pw_episode_log_absorb`` refuses on the host."""
import ctypes as C
import os
import pickle
import re

import numpy as np
import pytest
import torch

from multiagent_rl_amd import _lib
from multiagent_rl_amd.rollout import EpisodeLedger
from multiagent_rl_amd.train import (ChunkLedger, EpisodeLog, evaluate_batched, merge_histories, merge_histories_chronological,
                                     train_batched)
from tests import episode_log_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------
# the model
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,T,N', [(1, 7, 3), (2, 2, 1), (5, 1, 3), (9, 7, 6), (65, 26, 3)])
def test_the_case_generator_keeps_its_promises(B, T, N):
    ref.assert_case_conditions(ref.synthetic_case(B, T, N))
    ref.assert_case_conditions(ref.synthetic_case(B, T, N, quantised=True))
    if B >= 2:
        case = ref.synthetic_case(B, T, N, calls=4, kinds=('mixed', 'none', 'all', 'mixed'))
        ref.assert_case_conditions(case)
        m, snaps = ref.run_model(case, ref.capacity_for(case))
        assert snaps[1]['length'] == snaps[0]['length'] and snaps[2]['length'] == snaps[1]['length'] + T * B
        assert snaps[1]['step_base'] == snaps[0]['step_base'] + T


def test_model_slots_capacity_and_carry_by_hand():
    """Two envs, two agents, written out: the order of the entries, the total as a sum of its own, the carry by assignment, an entry
    past the capacity that is dropped while length and carry go on."""
    rew = np.array([[[1.0, 2.0], [10.0, 20.0]], [[4.0, 8.0], [40.0, 80.0]], [[0.5, 0.25], [5.0, 2.5]]], np.float32)   # [T=3, B=2, N=2]
    term = np.array([[0, 1], [1, 1], [0, 0]], bool)
    m = ref.EpisodeLogModel(2, 2, capacity=2)
    m.absorb(rew, term)
    assert (m.length, m.step_base) == (3, 3)                       # three episodes finished, two stored
    assert m.total[:2] == [30.0, 15.0] and m.by_agent[:2] == [[10.0, 20.0], [5.0, 10.0]]       # (t=0, e=1), then (t=1, e=0)
    assert m.end_step[:2] == [0, 1] and m.env[:2] == [1, 0]
    assert m.carry == [[0.5, 0.25, 0.75], [5.0, 2.5, 7.5]]         # the dropped entry (t=1, e=1) cleared env 1's sums all the same
    with pytest.raises(RuntimeError, match='overflowed'):
        m.entries()
    # a NaN poisons its own episode: share and total of that entry, nothing behind the flag
    rew2 = rew.copy()
    rew2[0, 0, 1] = np.nan
    p = ref.EpisodeLogModel(2, 2, capacity=8)
    p.absorb(rew2, term)
    assert np.isnan(p.total[1]) and np.isnan(p.by_agent[1][1]) and p.by_agent[1][0] == 5.0
    assert p.total[0] == 30.0 and p.total[2] == 120.0 and p.carry == [[0.5, 0.25, 0.75], [5.0, 2.5, 7.5]]
    # -0.0 rewards after a flag: the carry was ASSIGNED +0.0, and +0.0 + -0.0 = +0.0
    z = ref.EpisodeLogModel(1, 1, capacity=4)
    z.absorb(np.array([[[1.0]], [[-0.0]]], np.float32), np.array([[1], [0]], bool))
    assert z.carry == [[0.0, 0.0]] and not np.signbit(z.carry[0][0])


def test_model_is_the_b1_loops_ledger():
    """At B = 1 the model's lists are those of ``rollout.EpisodeLedger`` (the B = 1 host loop's accounting, run.py:55-65), entry for
    entry and bit for bit, the trailing open entry included -- whatever the chunking."""
    case = ref.synthetic_case(1, 26, 3, calls=4)
    rew, term = case['rew'], case['terminal']
    led = EpisodeLedger(3, window=10)
    for c in range(4):
        for t in range(26):
            led.credit([float(x) for x in rew[c, t, 0]])
            if term[c, t, 0]:
                led.open_next()
    m = ref.EpisodeLogModel(1, 3, capacity=200)
    for c in range(4):
        m.absorb(rew[c], term[c])
    want, got = led.history(), m.history(include_open=True)
    assert len(got['reward_episodes']) == int(term.sum()) + 1 > 3
    assert [float(x).hex() for x in got['reward_episodes']] == [float(x).hex() for x in want['reward_episodes']]
    for i in range(3):
        assert [float(x).hex() for x in got['reward_episodes_by_agents'][i]] == [float(x).hex() for x in want['reward_episodes_by_agents'][i]]
    assert m.history(include_open=False)['episode_end_step'] == [int(i) for i in np.flatnonzero(term.reshape(-1))]


@pytest.mark.parametrize('B,T,N', [(9, 7, 3), (65, 26, 6), (2, 2, 1)])
def test_model_against_chunk_ledger(B, T, N):
    """``ChunkLedger`` (the torch pipeline ``train_batched`` uses today) and the model over three chunks, both from a zero carry.  On
    rewards that are multiples of 2**-10 with |r| <= 2**10 every float64 sum is exact whatever its order: the two histories are EQUAL.  On
    log-uniform rewards each entry agrees within ``pair_bound`` of that entry's own terms."""
    q = ref.synthetic_case(B, T, N, quantised=True)
    led, m = ChunkLedger(B, N, 'cpu'), ref.EpisodeLogModel(B, N, capacity=int(q['terminal'].sum()))
    for c in range(3):
        led.absorb(torch.from_numpy(q['rew'][c]), torch.from_numpy(q['terminal'][c]))
        m.absorb(q['rew'][c], q['terminal'][c])
    assert led.history() == m.history(include_open=True)
    assert led.history(include_open=False)['reward_episodes'] == m.history(include_open=False)['reward_episodes']
    assert led.mean_of_last(5) == m.mean_of_last(5)

    case = ref.synthetic_case(B, T, N)
    led, m = ChunkLedger(B, N, 'cpu'), ref.EpisodeLogModel(B, N, capacity=int(case['terminal'].sum()))
    for c in range(3):
        led.absorb(torch.from_numpy(case['rew'][c]), torch.from_numpy(case['terminal'][c]))
        m.absorb(case['rew'][c], case['terminal'][c])
    got, want = led.history(), m.history(include_open=True)
    n = len(m)
    assert got['open_episodes'] == want['open_episodes'] == B and len(got['reward_episodes']) == len(want['reward_episodes']) == n + B
    worst = 0.0
    for k in range(n + B):
        terms = m.terms[k] if k < n else m.carry_terms[k - n]
        mags = m.abs_sum[k] if k < n else m.carry_abs[k - n]
        for i in range(N + 1):
            a = got['reward_episodes'][k] if i == N else got['reward_episodes_by_agents'][i][k]
            b = want['reward_episodes'][k] if i == N else want['reward_episodes_by_agents'][i][k]
            tol = ref.pair_bound(terms[i], mags[i])
            worst = max(worst, abs(a - b) / tol if tol else float(a != b))
            assert abs(a - b) <= tol, (k, i, a, b, tol)
    print('ChunkLedger against the model, B=%d T=%d N=%d: worst |diff| / pair_bound = %.3g over %d entries' % (B, T, N, worst, n + B))


# ------------------------------------------------------------------------------------------
# the chronological merge
# ------------------------------------------------------------------------------------------
def _part(B, N, ends, rank, with_open):
    """A rank's history: ``ends`` = [(end_step, env)] in log order; the return of an episode encodes who it was."""
    tot = [1000.0 * rank + 10.0 * s + e for s, e in ends]
    h = {'reward_episodes': list(tot), 'reward_episodes_by_agents': [[x + 0.1 * (i + 1) for x in tot] for i in range(N)],
         'open_episodes': 0, 'episode_end_step': [s for s, _ in ends], 'episode_env': [e for _, e in ends], 'num_envs': B}
    if with_open:
        h['open_episodes'] = B
        h['reward_episodes'] += [-(100.0 * rank + e) for e in range(B)]
        for i in range(N):
            h['reward_episodes_by_agents'][i] += [-(100.0 * rank + e) - 0.1 * (i + 1) for e in range(B)]
    return h


@pytest.mark.parametrize('with_open', [False, True])
def test_merge_histories_chronological_interleaves_three_ranks(with_open):
    """Three ranks of B = 3 envs with interleaved end steps and ties: sorted by (end step, rank, env), the rank and the global env id
    beside every entry, the open returns behind them in global env order, ONE open count, the per-rank counts kept."""
    B, N = 3, 2
    ends = [[(4, 1), (9, 0), (9, 2), (30, 1)],                   # rank 0
            [(2, 2), (9, 0), (9, 1), (12, 0), (30, 0)],          # rank 1: ties with rank 0 at steps 9 and 30
            [(9, 1), (10, 0)]]                                   # rank 2
    parts = [_part(B, N, e, r, with_open) for r, e in enumerate(ends)]
    got = merge_histories_chronological(parts)
    want = sorted((s, r, e) for r, es in enumerate(ends) for s, e in es)
    n = len(want)
    assert n == 11 and got['episode_end_step'] == [s for s, _, _ in want] and got['episode_rank'] == [r for _, r, _ in want]
    assert got['episode_env'] == [r * B + e for _, r, e in want]
    assert got['reward_episodes'][:n] == [1000.0 * r + 10.0 * s + e for s, r, e in want]
    for i in range(N):
        assert got['reward_episodes_by_agents'][i][:n] == [1000.0 * r + 10.0 * s + e + 0.1 * (i + 1) for s, r, e in want]
    assert got['episodes_per_rank'] == [4, 5, 2]
    if with_open:
        assert got['open_episodes'] == 3 * B and got['reward_episodes'][n:] == [-(100.0 * r + e) for r in range(3) for e in range(B)]
        assert got['reward_episodes_by_agents'][1][n:] == [-(100.0 * r + e) - 0.2 for r in range(3) for e in range(B)]
    else:
        assert got['open_episodes'] == 0 and len(got['reward_episodes']) == n
    assert all(len(x) == len(got['reward_episodes']) for x in got['reward_episodes_by_agents'])
    # the rank-order merge is what it was
    old = merge_histories(parts)
    assert old['reward_episodes'] == [x for p in parts for x in p['reward_episodes']] and old['open_episodes'] == [p['open_episodes'] for p in parts]
    bad = [dict(p) for p in parts]
    bad[1]['episode_env'] = bad[1]['episode_env'][:-1]
    with pytest.raises(ValueError, match='rank 1'):
        merge_histories_chronological(bad)


# ------------------------------------------------------------------------------------------
# control flow with stubs
# ------------------------------------------------------------------------------------------
class _Args(object):
    max_episode_len, num_episodes, is_training = 5, 20, True
    batch_size, warmup_steps, update_rate, save_rate, display = 8, 64, 16, 8, False
    appx = 'PREFIX_'


class _Space(object):
    def __init__(self, n):
        self.n, self.shape = n, (10,)


class _StubEnv(object):
    num_envs, n, obs_dim = 8, 3, 10
    observation_space = [_Space(5)] * 3
    action_space = [_Space(5)] * 3


class _StubTrainer(object):
    trace = None

    def __init__(self, actor, critic, memory, action_type='Discrete'):
        self.actor, self.memory = actor, memory
        self.trace.append(('trainer_init', action_type))

    def optimize(self):
        self.trace.append(('optimize',))

    def save_models(self, name):
        self.trace.append(('save_models', name))

    def load_models(self, name):
        self.trace.append(('load_models', name))


class _StubMemory(object):
    n = 0

    def __len__(self):
        return self.n


def _stub_planes(step0, T, B, N):
    """Env e's clock starts at e % 5 and ends an episode every 5 steps (desynchronised); the reward names (step, env, agent)."""
    t = torch.arange(step0, step0 + T)
    term = ((t[:, None] + torch.arange(B)[None, :]) % 5) == 4
    rew = -(t[:, None, None] * 1.0 + torch.arange(B)[None, :, None] * 0.125 + torch.arange(N)[None, None, :] * 0.015625).float()
    return rew.contiguous(), term.contiguous()


class _StubFused(object):
    """FusedActor's surface as evaluate_batched uses it: ``rollout`` fills the caller's ``out`` and the statistics."""

    def __init__(self, trace):
        self.trace, self.steps = trace, 0

    def refresh(self):
        self.trace.append(('refresh',))

    def rollout(self, env, num_steps, out=None, memory=None, stats=None):
        assert set(out) == {'rew', 'terminal', 'act'} and out['act'] is None       # only what the library serves and the log needs
        rew, term = _stub_planes(self.steps, num_steps, env.num_envs, env.n)
        out['rew'].copy_(rew)
        out['terminal'].copy_(term)
        self.steps += num_steps
        stats[2].add_(int(term.sum()))
        stats[1].add_(float(rew.double().sum(2)[term].sum()))
        self.trace.append(('rollout', num_steps, memory is not None))
        return out


class _StubRollout(object):
    def __init__(self, env, memory, trace):
        self.env, self.memory, self.trace = env, memory, trace
        self.obs = torch.zeros(env.num_envs, env.n, env.obs_dim)
        self.env_steps, self.steps = 0, 0
        self.episode_return = torch.zeros(env.num_envs)
        self.finished_return_sum = torch.zeros((), dtype=torch.float64)
        self.finished_episodes = torch.zeros((), dtype=torch.int64)

    def collect_one_launch(self, num_steps, chunk=100, keep_outputs=False):
        B, N = self.env.num_envs, self.env.n
        rew, term = _stub_planes(self.steps, num_steps, B, N)
        self.trace.append(('collect', num_steps, keep_outputs))
        self.last_chunk = dict(rew=rew, terminal=term)
        self.steps += num_steps
        self.env_steps += num_steps * B
        self.memory.n += num_steps * B
        self.finished_episodes += int(term.sum())

    def stats(self):
        n = float(self.finished_episodes)
        return dict(env_steps=self.env_steps, episodes=int(n), mean_episode_reward=float(self.finished_return_sum) / n if n else float('nan'))


def test_evaluate_batched_control_flow(tmp_path):
    """``evaluate_batched`` with a stub Trainer, a stub rollout and the model as the log: the models are loaded under the reference's
    name and never saved, ``optimize`` is never called, each chunk is one rollout launch of ``max_episode_len`` steps whose ``out`` holds
    rew / terminal only, the loop stops at the FIRST chunk that reaches ``num_episodes``, the history holds finished episodes only and
    is written as ``test_history_...``."""
    trace, logs, made = [], [], []
    _StubTrainer.trace = trace
    env, cfg = _StubEnv(), _Args()

    def make_ledger(*a):
        made.append(ref.EpisodeLogModel(*a))
        return made[-1]

    hist = evaluate_batched(env, 'actor', 'critic', _StubTrainer, 'simple_spread', 'Discrete', cnt=3, arglist=cfg, out_dir=str(tmp_path),
                            log=lambda *a: logs.append(a), make_ledger=make_ledger,
                            make_rollout=lambda e, actor, memory, seed: (_StubFused(trace), _StubRollout(e, memory, trace)))
    kinds = [e[0] for e in trace]
    assert trace[0] == ('trainer_init', 'Discrete') and trace[1] == ('load_models', 'PREFIX_simple_spread_fin_3')
    assert 'save_models' not in kinds and 'optimize' not in kinds and 'refresh' not in kinds
    # 8 envs, one end per env and 5-step chunk: 8 episodes per chunk -> 20 is first reached by the third chunk
    assert trace[2:] == [('rollout', 5, False)] * 3
    log = made[0]
    assert (log.B, log.N) == (8, 3) and log.capacity == 20 + 8 * (5 // 5 + 2) and len(log) == 24
    assert sorted(hist) == ['episode_end_step', 'episode_env', 'open_episodes', 'reward_episodes', 'reward_episodes_by_agents', 'stats']
    assert hist['open_episodes'] == 0 and len(hist['reward_episodes']) == 24 and [len(x) for x in hist['reward_episodes_by_agents']] == [24] * 3
    assert hist['episode_end_step'] == sorted(hist['episode_end_step']) and hist['episode_end_step'][0] == 0 and hist['episode_end_step'][-1] == 14
    assert hist['episode_env'][:3] == [4, 3, 2]                  # clocks start at e % 5: env 4 ends on step 0, env 3 on step 1, ...
    # an entry is the sum of its episode's rewards: env 4's first episode is the single step 0
    assert hist['reward_episodes'][0] == sum(-(0.0 + 4 * 0.125 + a * 0.015625) for a in range(3))
    st = hist['stats']
    assert (st['env_steps'], st['episodes'], st['updates'], st['chunk'], st['num_envs'], st['world']) == (120, 24, 0, 5, 8, 1)
    assert os.listdir(tmp_path) == ['test_history_simple_spread_3.pkl']
    saved = pickle.load(open(tmp_path / 'test_history_simple_spread_3.pkl', 'rb'))
    assert saved['reward_episodes'] == hist['reward_episodes'] and 'memory' not in saved
    lines = [a[0] for a in logs if 'mean episode reward' in str(a[0])]
    assert len(lines) == 3 and lines[-1].startswith('steps: 120, episodes: 24, mean episode reward: %s, time: ' % np.mean(hist['reward_episodes'][-10:]))
    # model_prefix and memory: the name loaded, the ring sink requested, the memory in the history; a larger chunk
    trace.clear()
    mem = _StubMemory()
    h2 = evaluate_batched(env, 'actor', 'critic', _StubTrainer, 'simple_spread', 'Discrete', cnt=0, arglist=cfg, memory=mem, out_dir=None,
                          log=lambda *a: None, chunk=12, model_prefix='', make_ledger=ref.EpisodeLogModel,
                          make_rollout=lambda e, actor, memory, seed: (_StubFused(trace), _StubRollout(e, memory, trace)))
    assert trace[1] == ('load_models', 'simple_spread_fin_0') and trace[2:] == [('rollout', 12, True)] * 2
    assert h2['memory'] is mem and h2['stats']['env_steps'] == 2 * 12 * 8 and len(h2['reward_episodes']) == h2['stats']['episodes'] >= 20
    with pytest.raises(ValueError, match='action_type'):
        evaluate_batched(env, 'actor', 'critic', _StubTrainer, 'simple_spread', 'Continuous', arglist=cfg)


def test_train_batched_device_ledger_control_flow(tmp_path):
    """``train_batched(ledger='device')`` with the model in the log's place against the same run with ``ledger='host'``: the same
    launches, updates and refreshes, the same report lines, the same history (the stub's rewards are multiples of 2**-6: every float64
    sum is exact), the log built with ``num_episodes + B (chunk // max_episode_len + 2)`` entries."""
    runs = {}
    for which in ('host', 'device'):
        trace, logs, made = [], [], []
        _StubTrainer.trace = trace
        env, cfg, mem = _StubEnv(), _Args(), _StubMemory()

        def make_ledger(*a):
            made.append(ref.EpisodeLogModel(*a))
            return made[-1]

        hist = train_batched(env, 'actor', 'critic', _StubTrainer, 'simple_spread', 'Discrete', cnt=1, arglist=cfg, memory=mem,
                             out_dir=str(tmp_path / which), log=lambda *a: logs.append(a), chunk=12, ledger=which, make_ledger=make_ledger,
                             make_rollout=lambda e, actor, memory, seed: (_StubFused(trace), _StubRollout(e, memory, trace)))
        runs[which] = (hist, trace, [a[0] for a in logs if 'mean episode reward' in str(a[0])], made)
    (h_host, t_host, l_host, m_host), (h_dev, t_dev, l_dev, m_dev) = runs['host'], runs['device']
    assert not m_host and len(m_dev) == 1 and m_dev[0].capacity == 20 + 8 * (12 // 5 + 2)
    assert t_host == t_dev and t_dev[-1] == ('save_models', 'simple_spread_fin_1') and ('optimize',) in t_dev
    strip = lambda s: s[:s.index(', time:')]  # noqa: E731
    assert l_dev and [strip(s) for s in l_host] == [strip(s) for s in l_dev]
    for k in ('reward_episodes', 'reward_episodes_by_agents', 'open_episodes'):
        assert h_host[k] == h_dev[k], k
    assert sorted(h_dev) == sorted(h_host) and h_dev['open_episodes'] == 8
    assert pickle.load(open(tmp_path / 'device' / 'history_simple_spread_1.pkl', 'rb'))['reward_episodes'] == h_dev['reward_episodes']
    with pytest.raises(ValueError, match='ledger'):
        train_batched(_StubEnv(), 'actor', 'critic', _StubTrainer, 'simple_spread', arglist=_Args(), memory=_StubMemory(), ledger='gpu')


# ------------------------------------------------------------------------------------------
# the ABI
# ------------------------------------------------------------------------------------------
def _valid_log():
    log = _lib.PwEpisodeLog()
    log.struct_size, log.num_envs, log.num_agents, log.capacity = C.sizeof(_lib.PwEpisodeLog), 64, 3, 100
    for i, (name, _) in enumerate(_lib.PwEpisodeLog._fields_[4:]):
        setattr(log, name, 4096 * (i + 1))                        # fake, aligned "device pointers": every call below is refused before a launch
    return log


def test_episode_log_arguments_are_checked_on_the_host():
    lib = _lib.load()
    p = C.c_void_p(1 << 20)

    def refused(edit, word, rew=p, term=p, T=10):
        log = _valid_log()
        edit(log)
        rc = lib.pw_episode_log_absorb(C.byref(log), rew, term, T, None)
        msg = lib.pw_last_error().decode()
        assert rc == -1 and word in msg, (rc, msg, word)

    refused(lambda l: setattr(l, 'struct_size', 80), 'struct_size')
    refused(lambda l: None, 'T must', T=0)
    refused(lambda l: setattr(l, 'num_envs', 0), 'num_envs')
    refused(lambda l: setattr(l, 'num_agents', 0), 'num_agents')
    refused(lambda l: setattr(l, 'num_agents', 97), 'num_agents')
    refused(lambda l: setattr(l, 'capacity', 0), 'capacity')
    refused(lambda l: setattr(l, 'num_envs', 1 << 22), 'slot plane', T=512)            # T * B = 2**31
    refused(lambda l: (setattr(l, 'num_envs', 1 << 26), setattr(l, 'num_agents', 96)), 'walk threads', T=1)   # B (N + 1) >= 2**32, T B fits
    refused(lambda l: None, 'rew is null', rew=None)
    refused(lambda l: None, 'terminal is null', term=None)
    refused(lambda l: None, 'rew must be 4-byte', rew=C.c_void_p((1 << 20) + 2))
    for name in ('total', 'by_agent', 'end_step', 'env', 'carry', 'length', 'step_base', 'scratch'):
        refused(lambda l: setattr(l, name, None), name + ' is null')
        refused(lambda l: setattr(l, name, getattr(l, name) + (2 if name == 'env' else 4)), name + ' must be')
    assert lib.pw_episode_log_absorb(None, p, p, 10, None) == -1 and b'log is null' in lib.pw_last_error()
    # the scratch: a header, one count per tile of 1024 flags, one int32 slot per flag, each on a 256-byte boundary
    assert lib.pw_episode_log_scratch_bytes(1, 1) == 3 * 256
    assert lib.pw_episode_log_scratch_bytes(100, 4096) == 256 + 1792 + 4 * 409600
    assert lib.pw_episode_log_scratch_bytes(0, 8) == lib.pw_episode_log_scratch_bytes(8, 0) == lib.pw_episode_log_scratch_bytes(512, 1 << 22) == 0
    assert lib.pw_episode_log_scratch_bytes(1, 0x7fffffff) > 0


def test_episode_log_struct_matches_the_header_and_the_integration_stub():
    hdr = open(os.path.join(ROOT, 'include', 'pworld.h')).read()
    body = hdr[hdr.index('typedef struct pw_episode_log {'):hdr.index('} pw_episode_log;')]
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    names = [n for decl in re.findall(r'^\s*[\w ]+?[ *]+([\w, ]+);', body, flags=re.M) for n in re.split(r',\s*', decl.strip())]
    assert names == [f[0] for f in _lib.PwEpisodeLog._fields_]
    assert C.sizeof(_lib.PwEpisodeLog) == 88                      # 4 + 4 + 4 (+ 4 padding) + 8 + 8 pointers
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    block = doc[doc.index('class pw_episode_log(C.Structure)'):]
    block = block[:block.index('```')]
    assert re.findall(r"\('(\w+)', C\.", block) == [f[0] for f in _lib.PwEpisodeLog._fields_]
    assert int(re.search(r'#define\s+PW_EPISODE_LOG_MAX_AGENTS\s+(\d+)', hdr).group(1)) == _lib.PW_EPISODE_LOG_MAX_AGENTS == 96


def test_episode_log_has_no_host_fallback():
    """The log is the HIP launch: asked for on the CPU it raises instead of computing something else."""
    with pytest.raises(_lib.PworldError, match='no CPU fallback'):
        EpisodeLog(4, 3, 16, 'cpu')
    with pytest.raises(ValueError, match='num_agents'):
        EpisodeLog(4, 97, 16, 'cpu')
