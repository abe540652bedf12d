"""GPU: pw_episode_log_absorb / train.EpisodeLog against the reference model (tests/episode_log_ref.py) BIT FOR BIT -- the entries, their
order, the carry and the two cells after each of three consecutive launches into one log; that chunking does not matter; repeatability;
overflow with canaries behind every array; non-finite rewards; the log on the planes of real one-launch rollouts against the model and
against the rollout's own statistics sink; ``train.evaluate_batched`` end to end and ``train_batched(ledger='device')`` against
``ledger='host'``.

The merge of several ranks' histories runs on the GPU in tests/test_gpu_episode_log_two_ranks.py (two ranks sharing the card) and on the
CPU in tests/test_episode_log_host.py and tests/test_episode_log_dist_gloo.py; no test in THIS file starts a child process."""
import ctypes as C
import os
import pickle
import sys

import numpy as np
import pytest
import torch

from tests import episode_ledger_ref as elr
from tests import episode_log_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def _log_for(case, capacity):
    """An EpisodeLog in the state the case starts from (non-zero carry, length and step count)."""
    from multiagent_rl_amd.train import EpisodeLog
    _, T, B, N = case['rew'].shape
    log = EpisodeLog(B, N, capacity, DEV)
    log.carry.copy_(torch.from_numpy(case['carry0']))
    log.cells.copy_(torch.tensor([case['length0'], case['step_base0']]))
    return log


def _absorb(log, rew, term):
    log.absorb(torch.from_numpy(np.ascontiguousarray(rew)).to(DEV), torch.from_numpy(np.ascontiguousarray(term)).to(DEV))


def _assert_log_is(log, snap, label, lo=0):
    """Every array, the carry and the cells of ``log`` against a model snapshot, bit for bit; the slots in [lo, first) and behind the
    stored part are untouched (zero)."""
    first, n = snap['first'], snap['stored']
    cells = log.cells.cpu().numpy()
    assert (int(cells[0]), int(cells[1])) == (snap['length'], snap['step_base']), (label, cells, snap['length'], snap['step_base'])
    total, by = log.total.cpu().numpy(), log.by_agent.cpu().numpy()
    assert np.array_equal(log.end_step.cpu().numpy()[first:n], snap['end_step']), label + ': end_step'
    assert np.array_equal(log.env.cpu().numpy()[first:n], snap['env']), label + ': env'
    assert np.array_equal(_bits(total[first:n]), _bits(snap['total'])), '%s: total differs at %s' % (
        label, np.flatnonzero(_bits(total[first:n]) != _bits(snap['total']))[:8])
    assert np.array_equal(_bits(by[first:n]), _bits(snap['by_agent'])), '%s: by_agent differs at %s' % (
        label, np.argwhere(_bits(by[first:n]) != _bits(snap['by_agent']))[:8])
    assert np.array_equal(_bits(log.carry.cpu().numpy()), _bits(snap['carry'])), label + ': carry'
    assert not _bits(total[lo:first]).any() and not _bits(total[n:]).any() and not _bits(by[n:]).any(), label + ': a slot outside the launch was written'


CASES = [(B, T, N) for B in (1, 63, 64, 65, 257, 1025) for T in (1, 2, 7, 26) for N in (1, 3, 6)] + [(65, 7, 50)]


@pytest.mark.parametrize('B,T,N', CASES)
def test_kernel_against_the_model_bit_for_bit(B, T, N):
    """Three consecutive launches into one log that starts from a non-zero carry, length and step count: after EACH the log equals the
    model -- total and by_agent as uint64, end_step, env, carry, length, step_base.  B around the wave and workgroup sizes and over
    several workgroups, T = 1 (every flag is a first and a last step) to 26, N = 1 (share = total), 3, 6 and 50."""
    case = ref.synthetic_case(B, T, N)
    ref.assert_case_conditions(case)
    cap = ref.capacity_for(case) + 3
    _, snaps = ref.run_model(case, cap)
    log = _log_for(case, cap)
    for c in range(3):
        _absorb(log, case['rew'][c], case['terminal'][c])
        _assert_log_is(log, snaps[c], 'B=%d T=%d N=%d launch %d' % (B, T, N, c))
    assert len(log) == snaps[-1]['length'] and snaps[-1]['length'] > case['length0']


def test_a_launch_without_a_flag_and_one_with_every_flag():
    case = ref.synthetic_case(65, 7, 3, calls=4, kinds=('mixed', 'none', 'all', 'mixed'))
    ref.assert_case_conditions(case)
    cap = ref.capacity_for(case)
    _, snaps = ref.run_model(case, cap)
    log = _log_for(case, cap)
    for c in range(4):
        _absorb(log, case['rew'][c], case['terminal'][c])
        _assert_log_is(log, snaps[c], 'kinds launch %d (%s)' % (c, case['kinds'][c]))


@pytest.mark.parametrize('B,T,N', [(65, 7, 3), (257, 13, 6)])
def test_chunking_does_not_matter(B, T, N):
    """One launch over the [2T] planes and two launches over their halves leave the same log, bit for bit."""
    case = ref.synthetic_case(B, 2 * T, N, calls=1, seed=3)
    cap = ref.capacity_for(case)
    whole, halves = _log_for(case, cap), _log_for(case, cap)
    _absorb(whole, case['rew'][0], case['terminal'][0])
    _absorb(halves, case['rew'][0][:T], case['terminal'][0][:T])
    _absorb(halves, case['rew'][0][T:], case['terminal'][0][T:])
    for name in ('total', 'by_agent', 'end_step', 'env', 'carry', 'cells'):
        a, b = getattr(whole, name).cpu().numpy(), getattr(halves, name).cpu().numpy()
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), name
    assert len(whole) == cap > case['length0']
    _assert_log_is(whole, ref.run_model(case, cap)[1][0], 'whole')


def test_the_same_launch_gives_the_same_bits():
    """The same launch from the same state twice, and once more after an unrelated launch (another shape, its own scratch) in between."""
    case = ref.synthetic_case(257, 26, 6, calls=1, seed=5)
    other = ref.synthetic_case(63, 7, 3, calls=1, seed=6)
    cap = ref.capacity_for(case)
    got = []
    for i in range(3):
        log = _log_for(case, cap)
        if i == 2:
            _absorb(_log_for(other, ref.capacity_for(other)), other['rew'][0], other['terminal'][0])
        _absorb(log, case['rew'][0], case['terminal'][0])
        got.append({n: getattr(log, n).cpu().numpy().copy() for n in ('total', 'by_agent', 'end_step', 'env', 'carry', 'cells')})
    for i in (1, 2):
        for n in got[0]:
            assert np.array_equal(got[0][n].view(np.uint8), got[i][n].view(np.uint8)), (i, n)
    # the same log object again, state put back: its scratch is reused
    log = _log_for(case, cap)
    _absorb(log, case['rew'][0], case['terminal'][0])
    log.carry.copy_(torch.from_numpy(case['carry0']))
    log.cells.copy_(torch.tensor([case['length0'], case['step_base0']]))
    _absorb(log, case['rew'][0], case['terminal'][0])
    assert np.array_equal(log.total.cpu().numpy().view(np.uint8), got[0]['total'].view(np.uint8))


def test_overflow_stores_nothing_past_the_arrays():
    """Capacity below the number of finished episodes, through the C ABI with canary words behind every array: the first ``capacity``
    entries are right, every canary is intact, ``length`` counts all episodes and the carry is what it would have been; ``entries()`` of
    the Python log raises."""
    from multiagent_rl_amd import _lib
    from multiagent_rl_amd.train import EpisodeLog
    B, T, N = 65, 7, 3
    case = ref.synthetic_case(B, T, N)
    full = ref.capacity_for(case)
    cap = case['length0'] + int(case['terminal'][0].sum()) + 5         # the second launch runs over, the third is past it altogether
    assert cap < full - int(case['terminal'][2].sum())
    m, snaps = ref.run_model(case, cap)
    lib, PAD, CANARY = _lib.load(), 64, 0x5A
    sizes = dict(total=cap * 8, by_agent=cap * N * 8, end_step=cap * 8, env=cap * 4, carry=B * (N + 1) * 8, cells=16,
                 scratch=lib.pw_episode_log_scratch_bytes(T, B))
    buf = {k: torch.full((n + PAD,), CANARY, dtype=torch.uint8, device=DEV) for k, n in sizes.items()}
    for k in ('total', 'by_agent', 'end_step', 'env'):
        buf[k][:sizes[k]] = 0
    buf['carry'][:sizes['carry']] = torch.from_numpy(case['carry0'].reshape(-1).view(np.uint8)).to(DEV)
    buf['cells'][:16] = torch.from_numpy(np.array([case['length0'], case['step_base0']], np.int64).view(np.uint8)).to(DEV)
    log = _lib.PwEpisodeLog()
    log.struct_size, log.num_envs, log.num_agents, log.capacity = C.sizeof(log), B, N, cap
    for k in ('total', 'by_agent', 'end_step', 'env', 'carry', 'scratch'):
        setattr(log, k, buf[k].data_ptr())
    log.length, log.step_base = buf['cells'].data_ptr(), buf['cells'].data_ptr() + 8
    for c in range(3):
        rew, term = torch.from_numpy(case['rew'][c]).to(DEV), torch.from_numpy(case['terminal'][c]).to(DEV)
        _lib.check(lib.pw_episode_log_absorb(C.byref(log), _lib.ptr(rew), _lib.ptr(term), T, _lib.stream(torch.device(DEV))))
    torch.cuda.synchronize()
    host = {k: v.cpu().numpy() for k, v in buf.items()}
    for k, n in sizes.items():
        assert (host[k][n:] == CANARY).all(), 'the canary behind %s was overwritten' % k
    snap = snaps[-1]
    cells = host['cells'][:16].view(np.int64)
    assert int(cells[0]) == snap['length'] == full > cap and int(cells[1]) == snap['step_base'] and snap['stored'] == cap
    first = snap['first']
    assert np.array_equal(host['total'][:cap * 8].view(np.uint64)[first:], _bits(snap['total']))
    assert np.array_equal(host['by_agent'][:cap * N * 8].view(np.uint64).reshape(cap, N)[first:], _bits(snap['by_agent']))
    assert np.array_equal(host['end_step'][:cap * 8].view(np.int64)[first:], snap['end_step'])
    assert np.array_equal(host['env'][:cap * 4].view(np.int32)[first:], snap['env'])
    assert np.array_equal(host['carry'][:sizes['carry']].view(np.uint64).reshape(B, N + 1), _bits(snap['carry']))
    # the Python log: length > capacity is an error, not a truncated history
    plog = EpisodeLog(B, N, 4, DEV)
    _absorb(plog, case['rew'][0], case['terminal'][0])
    assert len(plog) == int(case['terminal'][0].sum()) > 4
    for call in (plog.entries, plog.history, lambda: plog.mean_of_last(3)):
        with pytest.raises(RuntimeError, match='overflowed'):
            call()


def test_a_non_finite_reward_poisons_its_own_episode_only():
    """One NaN and one Inf reward in two (env, agent) places: exactly those episodes' by_agent column and total are non-finite -- the
    model's mask --, every other entry keeps the bits of the clean launch, and the next episode of the same env is clean."""
    B, T, N = 65, 26, 3
    case = ref.synthetic_case(B, T, N, calls=1, seed=9)
    term = case['terminal'][0]
    dirty = case['rew'][0].copy()
    places = []
    thrice = next(e for e in range(1, B - 1) if term[:, e].sum() >= 3)     # an env with an episode behind the poisoned one
    for value, e, a in ((np.nan, 0, 1), (np.inf, thrice, 2)):
        ends = np.flatnonzero(term[:, e])
        assert len(ends) >= 2, 'the env must finish twice: the episode behind the poisoned one is checked too'
        t = int(ends[0]) + 1                                    # inside the env's SECOND episode
        assert t <= ends[1]
        dirty[t, e, a] = value
        places.append((e, a, int(ends[1])))
    cap = ref.capacity_for(case)
    clean, bad = _log_for(case, cap), _log_for(case, cap)
    _absorb(clean, case['rew'][0], term)
    _absorb(bad, dirty, term)
    want = ref.EpisodeLogModel(B, N, cap, carry=case['carry0'], length=case['length0'], step_base=case['step_base0'])
    want.absorb(dirty, term)
    _assert_log_is(bad, want.snapshot(), 'poisoned launch')
    lo = case['length0']
    ct, cb = clean.total.cpu().numpy()[lo:], clean.by_agent.cpu().numpy()[lo:]
    bt, bb = bad.total.cpu().numpy()[lo:], bad.by_agent.cpu().numpy()[lo:]
    env, end = bad.env.cpu().numpy()[lo:], bad.end_step.cpu().numpy()[lo:] - case['step_base0']
    assert np.isfinite(ct).all() and np.isfinite(cb).all()
    mask_t, mask_b = np.zeros(len(bt), bool), np.zeros(bb.shape, bool)
    for e, a, t_end in places:
        k = np.flatnonzero((env == e) & (end == t_end))
        assert len(k) == 1
        mask_t[k[0]], mask_b[k[0], a] = True, True
    assert np.array_equal(~np.isfinite(bt), mask_t) and np.array_equal(~np.isfinite(bb), mask_b) and mask_t.sum() == 2
    assert np.array_equal(_bits(bt[~mask_t]), _bits(ct[~mask_t])) and np.array_equal(_bits(bb[~mask_b]), _bits(cb[~mask_b]))
    assert np.array_equal(_bits(bad.carry.cpu().numpy()), _bits(clean.carry.cpu().numpy()))       # both places lie before a flag
    for e, a, t_end in places:                                  # the same env's next episode, where it has one in this launch
        later = np.flatnonzero((env == e) & (end > t_end))
        assert np.isfinite(bt[later]).all() and np.isfinite(bb[later]).all() and (len(later) > 0 or e != thrice)


# ------------------------------------------------------------------------------------------
# on a real rollout
# ------------------------------------------------------------------------------------------
def _rollout_env(scenario, B, **kw):
    from multiagent_rl_amd import make_batched_env
    env = make_batched_env(scenario, B, auto_reset=True, max_episode_len=5, seed=21, **kw)
    env.reset()
    st = env.get_state()
    ep0 = (np.arange(B) % 5).astype(np.int32)                   # desynchronised episode clocks
    env.set_state(st['pos'], st['vel'], st['landmarks'], ep_step=ep0, ep_count=st['ep_count'])
    return env, ep0


@pytest.mark.parametrize('scenario,kw,B,N', [('simple_spread', dict(n=3), 130, 3), ('simple_reference', dict(), 65, 2)])
def test_log_of_a_real_rollout(scenario, kw, B, N):
    """Three one-launch rollouts of T = 12 (max_episode_len = 5, desynchronised clocks) with the statistics sink; the log absorbs each
    launch's own rew / terminal.  The log equals the model on those planes bit for bit; ``length`` equals the sink's ``finished_count``;
    ``sum(total)`` agrees with the sink's ``finished_sum`` within ``episode_ledger_ref.bound(n, abs_sum)`` with n and abs_sum derived as
    follows.  The sink adds up FLOAT32 returns: a reward reaches it through at most N - 1 float32 additions (the shared reward of the
    step), L = max_episode_len float32 additions of the running return, then float64 additions over the E finished returns; the log's
    path is N L float64 additions and the test's own sum E more.  One float32 rounding (u = 2**-24) is 2**29 float64 roundings' worth
    (U = 2**-53), so with every rounding counted in units of U both paths are sums of the same terms with at most
    n = (N - 1 + L) 2**29 + N L + 2 E roundings between a term and the result: |difference| <= gamma_n * abs_sum, abs_sum = the sum of
    |reward| over the finished episodes (the model counts it).  This is a plausibility check, NOT a tight cross-check: with float32 on the
    sink's side the bound is some 1e-2 where the difference is some 1e-4, so an error in one low-magnitude episode would pass it.  What
    carries the weight here is the bit-for-bit comparison with the model after every launch and ``length == finished_count``."""
    from multiagent_rl_amd.policy import ActorNetwork, FusedActor
    from multiagent_rl_amd.train import EpisodeLog
    T, L = 12, 5
    env, ep0 = _rollout_env(scenario, B, **kw)
    assert env.n == N
    torch.manual_seed(4)
    heads = [5, env.dim_c] if scenario == 'simple_reference' else 5
    actor = FusedActor(ActorNetwork(env.obs_dim, heads).cuda().eval(), seed=9)
    stats = (torch.zeros(B, device=DEV), torch.zeros((), dtype=torch.float64, device=DEV), torch.zeros((), dtype=torch.int64, device=DEV))
    cap = B * (3 * T // L + 1)
    log, model = EpisodeLog(B, N, cap, DEV), ref.EpisodeLogModel(B, N, cap)
    clocks = ep0
    for c in range(3):
        out = actor.rollout(env, T, stats=stats)
        term = out['terminal'].cpu().numpy()
        assert np.array_equal(term, elr.clock_terminals(clocks, T, L)), 'the episode clocks are not where set_state put them'
        clocks = (clocks + T) % L
        log.absorb(out['rew'], out['terminal'])
        model.absorb(out['rew'], out['terminal'])
        _assert_log_is(log, model.snapshot(), '%s launch %d' % (scenario, c))
    E = len(log)
    assert E == int(stats[2].item()) == model.length and E >= B * (3 * T // L)
    total = log.entries()['total']
    abs_sum = sum(model.abs_sum[k][N] for k in range(E))
    n = (N - 1 + L) * 2 ** 29 + N * L + 2 * E
    got, want = float(np.sum(total)), float(stats[1].item())
    print('%s: sum(total) %.17g, sink finished_sum %.17g, |diff| %.3g, bound %.3g (n = %d, abs_sum %.6g, %d episodes)'
          % (scenario, got, want, abs(got - want), elr.bound(n, abs_sum), n, abs_sum, E))
    assert abs(got - want) <= elr.bound(n, abs_sum)
    hist = log.history(include_open=False)
    assert hist['episode_end_step'] == sorted(hist['episode_end_step']) and hist['open_episodes'] == 0


# ------------------------------------------------------------------------------------------
# end to end
# ------------------------------------------------------------------------------------------
class _Cfg(object):
    max_episode_len, num_episodes, is_training = 5, 24, True
    batch_size, warmup_steps, update_rate, save_rate, display = 8, 40, 40, 8, False
    appx = 'unused_'


def _learner():
    sys.path.insert(0, os.path.join(ROOT, 'examples'))
    from madr_learner import CriticNetwork, Trainer
    return CriticNetwork, Trainer


def _env(B=8):
    from multiagent_rl_amd import make_batched_env
    return make_batched_env('simple_spread', B, n=3, auto_reset=True, max_episode_len=5, seed=12345678)


def test_evaluate_batched_end_to_end(tmp_path, monkeypatch):
    """A two-update training run saves its models; ``evaluate_batched`` loads them into fresh networks, plays 20 episodes on B = 8 envs
    in launches of 5 steps and pickles ``test_history_simple_spread_0.pkl``: chronological, at least 20 entries, none open -- and bit
    for bit the model applied to the planes of a second, identically seeded env + FusedActor rolled out by hand."""
    from multiagent_rl_amd.policy import ActorNetwork, FusedActor
    from multiagent_rl_amd.train import evaluate_batched, train_batched
    CriticNetwork, Trainer = _learner()
    monkeypatch.chdir(tmp_path)                                  # save_models / load_models: Models/ under the working directory
    torch.manual_seed(7)
    env = _env()
    trained = train_batched(env, ActorNetwork(env.obs_dim, 5), CriticNetwork(env.obs_dim + 5), Trainer, 'simple_spread', 'Discrete', cnt=0,
                            arglist=_Cfg(), out_dir=str(tmp_path / 'Models'), log=lambda *a: None, chunk=5)
    assert trained['stats']['updates'] == 2 and os.path.exists(tmp_path / 'Models' / 'simple_spread_fin_0_actor.pt')

    class Eval(_Cfg):
        num_episodes = 20

    lines = []
    env = _env()
    actor = ActorNetwork(env.obs_dim, 5)
    hist = evaluate_batched(env, actor, CriticNetwork(env.obs_dim + 5), Trainer, 'simple_spread', 'Discrete', cnt=0, arglist=Eval(),
                            out_dir=str(tmp_path / 'Models'), log=lambda *a: lines.append(a), model_prefix='')
    saved = pickle.load(open(tmp_path / 'Models' / 'test_history_simple_spread_0.pkl', 'rb'))
    assert saved['reward_episodes'] == hist['reward_episodes'] and 'memory' not in saved
    assert hist['open_episodes'] == 0 and len(hist['reward_episodes']) == 24 >= 20 and hist['stats']['episodes'] == 24
    assert hist['episode_end_step'] == sorted(hist['episode_end_step']) and hist['stats']['env_steps'] == 3 * 5 * 8
    assert len([a for a in lines if 'mean episode reward' in str(a[0])]) == 3
    # by hand: the same env seed, the loaded weights, the same policy seed
    env2 = _env()
    env2.reset()
    by_hand = ActorNetwork(env2.obs_dim, 5)
    by_hand.load_state_dict(torch.load(tmp_path / 'Models' / 'simple_spread_fin_0_actor.pt'))
    fused = FusedActor(by_hand.cuda(), seed=12345678)
    model = ref.EpisodeLogModel(8, 3, 64)
    for _ in range(3):
        out = fused.rollout(env2, 5)
        model.absorb(out['rew'], out['terminal'])
    want = model.history(include_open=False)
    for k in ('episode_end_step', 'episode_env'):
        assert hist[k] == want[k], k
    assert [float(x).hex() for x in hist['reward_episodes']] == [float(x).hex() for x in want['reward_episodes']]
    for i in range(3):
        assert [float(x).hex() for x in hist['reward_episodes_by_agents'][i]] == [float(x).hex() for x in want['reward_episodes_by_agents'][i]]


def test_train_batched_device_ledger_against_the_host_ledger(tmp_path, monkeypatch):
    """Two identically seeded ``train_batched`` runs (the learner never runs: the weights stay fixed), ``ledger='host'`` and
    ``ledger='device'``: the same ``reward_episodes`` / ``reward_episodes_by_agents``, entry for entry within ``pair_bound`` of the entry's
    own terms (both are float64 sums of the same float32 rewards, in different orders); the device run's log is the model on its planes."""
    from multiagent_rl_amd.policy import ActorNetwork
    from multiagent_rl_amd.train import EpisodeLog, train_batched
    CriticNetwork, Trainer = _learner()
    monkeypatch.chdir(tmp_path)

    class Cfg(_Cfg):
        num_episodes, warmup_steps = 300, 10 ** 9

    B, made = 37, []

    class Recording(EpisodeLog):
        """The log itself; its planes also go to the model."""

        def __init__(self, *a):
            super().__init__(*a)
            self.model = ref.EpisodeLogModel(self.B, self.N, self.capacity)
            made.append(self)

        def absorb(self, rew, terminal):
            super().absorb(rew, terminal)
            self.model.absorb(rew, terminal)

    hists = {}
    for which in ('host', 'device'):
        torch.manual_seed(11)
        env = _env(B)
        hists[which] = train_batched(env, ActorNetwork(env.obs_dim, 5), CriticNetwork(env.obs_dim + 5), Trainer, 'simple_spread', 'Discrete',
                                     cnt=0, arglist=Cfg(), out_dir=None, log=lambda *a: None, chunk=12, ledger=which, make_ledger=Recording)
    host, dev = hists['host'], hists['device']
    assert len(made) == 1 and host['stats']['updates'] == dev['stats']['updates'] == 0
    model = made[0].model
    assert made[0].capacity == 300 + B * (12 // 5 + 2)
    want = model.history(include_open=True)
    assert [float(x).hex() for x in dev['reward_episodes']] == [float(x).hex() for x in want['reward_episodes']]
    assert dev['open_episodes'] == host['open_episodes'] == B and len(dev['reward_episodes']) == len(host['reward_episodes']) >= 300 + B
    n = len(model)
    worst = 0.0
    for k in range(n + B):
        terms, mags = (model.terms[k], model.abs_sum[k]) if k < n else (model.carry_terms[k - n], model.carry_abs[k - n])
        for i in range(4):
            a = host['reward_episodes'][k] if i == 3 else host['reward_episodes_by_agents'][i][k]
            b = dev['reward_episodes'][k] if i == 3 else dev['reward_episodes_by_agents'][i][k]
            tol = ref.pair_bound(terms[i], mags[i])
            worst = max(worst, abs(a - b) / tol if tol else float(a != b))
            assert abs(a - b) <= tol, (k, i, a, b, tol)
    print('ledger host against device: worst |diff| / pair_bound = %.3g over %d entries' % (worst, n + B))
