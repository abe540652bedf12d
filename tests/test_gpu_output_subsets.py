"""GPU: pw_step / pw_rollout with a SUBSET of their optional outputs (include/pworld.h: "Any output pointer may be NULL (that output
is skipped)").

The dispatcher changes kernel on a missing output: launch_rollout (csrc/pworld.hip) takes the quad / duo / trio / stream / tag-duo
kernels only when obs, rew, rew_shared, done, terminal and act_idx are all present; one pointer less and the same handle runs
pw_spread_fast_kernel or the generic pw_rollout_kernel, whose every store is guarded on its own.  Per case, action form (int32 indices /
the equal float one-hot rows) and entry point (pw_step / a 7-step pw_rollout):

  * the full-set launch has the bits of the float32 C oracle (so that what follows does not rest on the library alone);
  * every subset -- the full set, the full set minus each name, each name alone, the four names dist.py hands over, and none at all --
    started from the same injected state with the same actions, leaves in every output it was given the bits of the full-set launch,
    and afterwards the same state (pos, vel, landmarks, ep_step, ep_count, comm, goal);
  * every output lives in a guarded buffer (tests/guarded.py): nothing is written around it;
  * where the full set runs a multi-wave or stream kernel, some subset ran another one (the fallback is really exercised).

Episodes of 3 steps with auto-reset; the injected episode clocks are staggered (ep_step = env % 3), so that within one wave some envs
reset in a step and others do not, a single pw_step resets a third of the batch, and every env resets at least twice in 7 steps.
No tolerance anywhere: bits, guard bytes, kernel names.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

from oracle import c_oracle as co  # noqa: E402  (checker only)
from tests.guarded import assert_guards_intact, guarded  # noqa: E402
from tests.test_gpu_parity import _assert_same_bits, _rand_state  # noqa: E402

T = 7
EP_LEN = 3
NAMES = ('obs', 'rew', 'rew_shared', 'done', 'terminal', 'final_obs', 'coll')
DIST_NAMES = ('obs', 'rew_shared', 'final_obs', 'terminal')      # what dist.py names

# id -> (scenario, kwargs of BatchedParticleEnv / co.make_config, dispatch override, B, a multi-wave / stream kernel serves the full set)
CASES = {
    'spread-N6-B13': ('simple_spread', dict(num_agents=6), {}, 13, True),                    # quad form; ragged last group of 8
    'spread-N3-B50': ('simple_spread', dict(num_agents=3), {}, 50, True),
    'spread-N3-B50-dense': ('simple_spread', dict(num_agents=3), dict(envs_per_wave=64), 50, True),
    'spread-N5-L2-B23': ('simple_spread', dict(num_agents=5, num_landmarks=2), {}, 23, True),   # run-time N
    'spread-N4-full-B9': ('simple_spread', dict(num_agents=4, obs_mode='full'), {}, 9, False),   # the generic kernel whatever is asked
    'spread-N64-B3': ('simple_spread', dict(num_agents=64), {}, 3, True),                    # collision mask bit 63
    'tag-3+1-B21': ('simple_tag', dict(num_agents=4, num_adversaries=3), {}, 21, True),
    'tag-2+3-L3-B11': ('simple_tag', dict(num_agents=5, num_adversaries=2, num_landmarks=3), {}, 11, True),
    'reference-B33': ('simple_reference', dict(num_agents=2), {}, 33, False),
    'speaker_listener-B33': ('simple_speaker_listener', dict(num_agents=2), {}, 33, False),     # 32 envs per workgroup plus one
}
ONE_WAVE = ('pw_spread_fast_kernel', 'pw_rollout_kernel')


def _np(t):
    return t.detach().cpu().numpy()


def _comm(scenario):
    return scenario in ('simple_reference', 'simple_speaker_listener')


def _names(scenario):
    return NAMES[:-1] if _comm(scenario) else NAMES      # coll only where the scenario has collisions


def _subsets(scenario):
    names = _names(scenario)
    subs = [names] + [tuple(n for n in names if n != x) for x in names] + [(x,) for x in names] + [DIST_NAMES, ()]
    return subs


def _sid(sub, scenario):
    names = _names(scenario)
    if sub == names:
        return 'all'
    if len(sub) == len(names) - 1:
        return 'all-but-' + [n for n in names if n not in sub][0]
    return '+'.join(sub) if sub else 'none'


def _make(case):
    from multiagent_rl_amd.env import BatchedParticleEnv
    scenario, kw, disp, B, _ = CASES[case]
    kw = dict(kw)
    N, A, om = kw.pop('num_agents'), kw.pop('num_adversaries', 0), kw.pop('obs_mode', 'local')
    ekw = dict(num_landmarks=kw.get('num_landmarks'), local_observation=om == 'local', max_episode_len=EP_LEN, auto_reset=True,
               seed=1234, env_id_base=7)
    if scenario == 'simple_tag':
        ekw.update(num_adversaries=A, num_good=N - A)
    elif scenario == 'simple_spread':
        ekw.update(num_agents=N)
    env = BatchedParticleEnv(scenario, B, dispatch=disp or None, **ekw)
    cfg = co.make_config(scenario, N, num_landmarks=kw.get('num_landmarks'), num_adversaries=A, obs_mode=om,
                         max_episode_len=EP_LEN, auto_reset=True, seed=1234, env_id_base=7)
    return env, cfg


@functools.lru_cache(maxsize=None)
def _inputs(case):
    """The injected state and the actions of a case, in both forms; drawn once, only read afterwards."""
    scenario, kw, _, B, _ = CASES[case]
    env, _ = _make(case)
    N, L = env.n, env.num_landmarks
    rng = np.random.RandomState(1000 + sorted(CASES).index(case))
    pos, vel, lm = _rand_state(rng, B, N, L)         # crowded: collisions and non-zero masks
    st = dict(pos=pos, vel=vel, landmarks=lm, ep_step=(np.arange(B) % EP_LEN).astype(np.int32),
              ep_count=(1 + np.arange(B) % 2).astype(np.int32))
    eye5 = np.eye(5, dtype=np.float32)
    if scenario == 'simple_reference':
        st.update(comm=np.eye(10, dtype=np.float32)[rng.randint(0, 10, (B, 2))], goal=rng.randint(0, 3, (B, 2)).astype(np.int32))
        idx = np.stack([rng.randint(0, 5, (T, B, 2)), rng.randint(0, 10, (T, B, 2))], -1).astype(np.int32)      # (movement, symbol)
        vec = np.concatenate([eye5[idx[..., 0]], np.eye(10, dtype=np.float32)[idx[..., 1]]], -1)
    elif scenario == 'simple_speaker_listener':
        st['vel'][:, 0] = 0                            # the speaker never moves
        goal = np.zeros((B, 2), np.int32)
        goal[:, 0] = rng.randint(0, 3, B)
        st.update(comm=np.zeros((B, 2, 3), np.float32), goal=goal)
        idx = np.stack([rng.randint(0, 3, (T, B)), rng.randint(0, 5, (T, B))], -1).astype(np.int32)   # (speaker's symbol, listener's move)
        vec = eye5[idx]                                # the speaker's vector lives in the first three entries
    else:
        idx = rng.randint(0, 5, (T, B, N)).astype(np.int32)
        vec = eye5[idx]
    return st, idx, vec


def _alloc(env, sub, lead):
    B, N, D = env.num_envs, env.n, env.obs_dim
    shapes = dict(obs=(B, N, D), final_obs=(B, N, D), rew=(B, N), rew_shared=(B,), done=(B, N), terminal=(B,), coll=(B, N))
    dtypes = dict(obs=torch.float32, final_obs=torch.float32, rew=torch.float32, rew_shared=torch.float32, done=torch.bool,
                  terminal=torch.bool, coll=torch.int64)
    return {n: guarded(lead + shapes[n], dtypes[n]) for n in sub}


def _launch(case, entry, form, sub):
    """One launch from the case's injected state -> (outputs as numpy, state afterwards as numpy, kernel name).  Guards checked here."""
    env, _ = _make(case)
    st, idx, vec = _inputs(case)
    env.set_state(st['pos'], st['vel'], st['landmarks'], ep_step=st['ep_step'], ep_count=st['ep_count'],
                  comm=st.get('comm'), goal=st.get('goal'))
    acts = torch.from_numpy(idx if form == 'idx' else vec)
    out = _alloc(env, sub, (T,) if entry == 'rollout' else ())
    if entry == 'rollout':
        env.rollout(acts, out)
    else:
        env.step(acts[0], out)
    torch.cuda.synchronize()
    kernel = env.last_kernel()
    for n, t in out.items():
        assert_guards_intact(t, '%s of subset {%s} (%s)' % (n, ', '.join(sub), kernel))
    after = {k: _np(v) for k, v in env.get_state().items()}
    return {n: _np(t) for n, t in out.items()}, after, kernel


@functools.lru_cache(maxsize=None)
def _full(case, entry, form):
    return _launch(case, entry, form, _names(CASES[case][0]))


def _oracle_steps(case, form, steps):
    """The float32 C oracle from the same state with the same actions -> (list of per-step output dicts, the oracle afterwards)."""
    scenario = CASES[case][0]
    _, cfg = _make(case)
    st, idx, vec = _inputs(case)
    B = CASES[case][3]
    if _comm(scenario):
        o = co.CRefOracle(cfg, B, np.float32)
        o.set_state(st['pos'], st['vel'], st['landmarks'], st['comm'], st['goal'])
        o.ep_step[...], o.ep_count[...] = st['ep_step'], st['ep_count']
    else:
        o = co.COracle(cfg, B, np.float32)
        o.set_state(st['pos'], st['vel'], st['landmarks'], st['ep_step'], st['ep_count'])
    ws = []
    for t in range(steps):
        if form == 'vec':
            w = o.step(act_vec=vec[t])
        elif scenario == 'simple_reference':
            w = o.step(act_idx=idx[t, ..., 0], act_comm=idx[t, ..., 1])
        else:
            w = o.step(act_idx=idx[t])
        if 'rew_shared' not in w:      # CRefOracle: run.py:46's agent-order sum, one float32 rounding per addition
            w['rew_shared'] = (np.float32(0) + w['rew'][:, 0]) + w['rew'][:, 1]
        ws.append(w)
    return ws, o


@pytest.mark.parametrize('form', ['idx', 'vec'])
@pytest.mark.parametrize('entry', ['step', 'rollout'])
@pytest.mark.parametrize('case', sorted(CASES))
def test_full_set_launch_has_the_oracles_bits(case, entry, form):
    scenario = CASES[case][0]
    out, after, kernel = _full(case, entry, form)
    steps = T if entry == 'rollout' else 1
    ws, o = _oracle_steps(case, form, steps)
    resets = masks = 0
    B, N = CASES[case][3], o.N
    self_bits = (np.uint64(1) << np.arange(N, dtype=np.uint64))[None, :]
    for t, w in enumerate(ws):
        sl = (lambda a: a[t]) if entry == 'rollout' else (lambda a: a)
        what = '%s [%s] step %d' % (case, kernel, t)
        for n in ('obs', 'rew', 'rew_shared'):
            _assert_same_bits(sl(out[n]), w[n], '%s: %s' % (what, n))
        _assert_same_bits(sl(out['done']).astype(np.uint8), w['done'], what + ': done')
        _assert_same_bits(sl(out['terminal']).astype(np.uint8), w['terminal'], what + ': terminal')
        ended = w['terminal'].astype(bool)
        assert np.array_equal(ended, (_inputs(case)[0]['ep_step'] + t + 1) % EP_LEN == 0), what
        resets += int(ended.sum())
        _assert_same_bits(sl(out['final_obs'])[ended], w['final_obs'][ended], what + ': final_obs of the envs that reset')
        if 'coll' in out:
            _assert_same_bits(sl(out['coll']).view(np.uint64), w['coll'], what + ': coll')
            masks += int((w['coll'] != self_bits).sum())
    # ep_step = env % 3: the envs with clock 2 end an episode in step 0 (and 3 and 6), the others twice in 7 steps
    assert resets == (2 * B + B // 3 if entry == 'rollout' else B // 3), (resets, B)
    if 'coll' in out and N > 1:
        assert masks > 0, 'the crowded state must exercise contacts'
    _assert_same_bits(after['pos'], o.pos, case + ': pos')
    _assert_same_bits(after['vel'], o.vel, case + ': vel')
    _assert_same_bits(after['landmarks'], o.lm, case + ': landmarks')
    assert np.array_equal(after['ep_step'], o.ep_step) and np.array_equal(after['ep_count'].astype(np.uint32), o.ep_count), case
    if _comm(scenario):
        _assert_same_bits(after['comm'], o.comm, case + ': comm')
        assert np.array_equal(after['goal'], o.goal), case


@pytest.mark.parametrize('form', ['idx', 'vec'])
@pytest.mark.parametrize('entry', ['step', 'rollout'])
@pytest.mark.parametrize('case', sorted(CASES))
def test_every_output_subset_equals_the_full_set_launch(case, entry, form):
    scenario, _, _, _, multi = CASES[case]
    want, want_after, full_kernel = _full(case, entry, form)
    kernels = {}
    for sub in _subsets(scenario):
        sid = _sid(sub, scenario)
        got, after, kernel = _launch(case, entry, form, sub)
        kernels[sid] = kernel
        what = '%s %s %s: subset %s ran %s, the full set %s' % (case, entry, form, sid, kernel, full_kernel)
        assert sorted(got) == sorted(sub), what
        for n in sub:      # whole buffers: final_obs rows of envs that did not reset keep the guard pattern in both
            _assert_same_bits(got[n], want[n], '%s: %s' % (what, n))
        assert sorted(after) == sorted(want_after), what
        for k in want_after:
            _assert_same_bits(after[k], want_after[k], '%s: state.%s afterwards' % (what, k))
    assert kernels['all'] == full_kernel, kernels
    if form == 'idx' and multi:
        # the full set is served by a multi-wave / stream kernel here, and a launch that leaves an output out must have left it
        assert not full_kernel.startswith(ONE_WAVE), kernels
        assert any(k != full_kernel for k in kernels.values()), kernels
        for sid, k in kernels.items():
            if sid.startswith('all-but-') and sid not in ('all-but-final_obs', 'all-but-coll'):
                assert k.startswith(ONE_WAVE), (sid, kernels)
    elif not multi or form == 'vec':
        # float actions, the full observation and the communication scenarios: one kernel whatever is asked
        assert len(set(k.split('<')[0] for k in kernels.values())) == 1, kernels
