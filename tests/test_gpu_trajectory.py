"""GPU: the HIP env FREE-RUNNING against the float64 oracle -- directly, not through the float32 one.

One ``env.rollout`` of T = 100 (four 25-step episodes with auto-reset) from ``env.reset()`` at the default dispatch, at the
shapes of tests/test_oracle_trajectory.py plus B = 1 and B = 5 at N = 6:
  * every structural assertion of the CPU test (tests/trajectory.py check_structure) on the HIP outputs: reset states equal to
    float64's, clocks identical, mask flips only inside the drift band, rewards inside their Lipschitz bound, contact-free envs
    inside the integrator's rounding bound;
  * the drift figures against the float32 C oracle's, computed on the host in the same run: at every step the kernel's max
    |dobs|, |drew|, |drew_shared| against float64 must not exceed the float32 oracle's.  Margin zero -- the project's contract is
    bit identity, so the two are the same numbers; a failure means a broken kernel or a broken bit-identity test;
  * two launches of 50 steps into one handle give the figures of one launch of 100;
  * simple_reference / simple_speaker_listener through their rollout entry and CRefOracle(float64);
  * the B = 1 drop-in under the reference's seed protocol (np.random.seed(12345678 + cnt), cnt 0 .. 9, N in {3, 6, 9, 12}, 25
    steps) against the Python float64 oracle env, with the same structural assertions.

PW_TRAJECTORY_REPORT=<path>: the per-step tables are appended there (profiles/trajectory_drift.txt holds such a run).
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

from oracle import c_oracle as co  # noqa: E402  (checker only)
from oracle import particle_oracle as po  # noqa: E402  (checker only)
from tests import trajectory as tj  # noqa: E402

# pw_dispatch_default(): every choice automatic
AUTO = dict(force_generic=0, no_stream=0, duo=-1, quad=-1, obs_block=-1, trio=-1, p_prio=-1, envs_per_wave=0, policy_form=0)

GPU_CASES = tj.CASES + [
    dict(id='spread6-B1', scenario='simple_spread', num_agents=6, B=1),
    dict(id='spread6-B5', scenario='simple_spread', num_agents=6, B=5),
]
IDS = [c['id'] for c in GPU_CASES]
_HIP = {}


def _np(t):
    return t.detach().cpu().numpy()


def _env(case, monkeypatch):
    from multiagent_rl_amd.env import BatchedParticleEnv
    for k in [k for k in os.environ if k.startswith('PWORLD_')]:
        monkeypatch.delenv(k)                                       # pw_create overlays them on the dispatch
    kw = dict(max_episode_len=tj.EP_LEN, auto_reset=True, seed=tj.SEED)
    if case['scenario'] == 'simple_spread':
        kw.update(num_agents=case['num_agents'], local_observation=case.get('obs_mode', 'local') == 'local')
    elif case['scenario'] == 'simple_tag':
        kw.update(num_adversaries=case['num_adversaries'], num_good=case['num_agents'] - case['num_adversaries'])
    comm = case['scenario'] in ('simple_reference', 'simple_speaker_listener')
    env = BatchedParticleEnv(case['scenario'], case['B'], want_coll=not comm, **kw)
    assert env.get_dispatch() == AUTO
    return env


def _hip_record(case, monkeypatch, chunks=(tj.T_FULL,)):
    """env.reset() + one rollout per chunk into ONE handle -> (recorded outputs as tests/trajectory.py takes them, kernel name)."""
    cfg = tj.config(case)
    env = _env(case, monkeypatch)
    acts = tj.actions(cfg, tj.T_FULL, case['B'])
    src = dict(obs0=_np(env.reset()))
    outs, t0, kernels = [], 0, set()
    for n in chunks:
        outs.append({k: _np(v) for k, v in env.rollout(torch.from_numpy(acts[t0:t0 + n])).items()})
        kernels.add(env.last_kernel())
        t0 += n
    assert t0 == tj.T_FULL and len(kernels) == 1
    for k in outs[0]:
        src[k] = np.concatenate([o[k] for o in outs])
    if 'coll' in src:
        src['coll'] = src['coll'].view(np.uint64)
    src['final_state'] = {k: _np(v) for k, v in env.get_state().items()}
    kernel = kernels.pop()
    assert kernel.startswith('pw_'), kernel                          # whatever pw_dispatch picked, by its own name
    return src, kernel


def _one_launch(case, monkeypatch):
    if case['id'] not in _HIP:
        _HIP[case['id']] = _hip_record(case, monkeypatch)
    return _HIP[case['id']]


def _device():
    return '%s %s' % (torch.cuda.get_device_name(0), getattr(torch.cuda.get_device_properties(0), 'gcnArchName', ''))


def _worst(d):
    return d.d_obs.max(axis=1), d.d_rew.max(axis=1), d.d_shared.max(axis=1)


@pytest.mark.parametrize('case', GPU_CASES, ids=IDS)
def test_hip_rollout_free_running_against_float64(case, monkeypatch):
    cfg = tj.config(case)
    o = tj.oracle_drift(case)                                        # float32 C oracle vs float64, on the host, this run
    src, kernel = _one_launch(case, monkeypatch)
    d = tj.drift(cfg, case['B'], o.acts, source=src, ref=o.ref)      # HIP vs float64: o.ref is the float64 record, nothing of the kernel's
    info = tj.check_structure(d)
    name = _device()
    tj.report(tj.table(d, 'gpu (%s) %s vs float64 C oracle: %s' % (name, kernel, case['id'])) + [tj.summary_line(case['id'], info)])
    assert info['resets'] == 5 and info['reset_states'] == 1
    for what, got, want in zip(('|dobs|', '|drew|', '|drew_shared|'), _worst(d), _worst(o)):
        over = got > want
        assert not over.any(), '%s: the kernel is further from float64 than the float32 oracle at steps %s (kernel %s, oracle %s)' % (
            what, np.nonzero(over)[0][:8].tolist(), got[over][:4].tolist(), want[over][:4].tolist())
    # the same split into contact / contact-free envs (decided on the float64 side alone)
    assert np.array_equal(d.contact, o.contact)


@pytest.mark.parametrize('case', GPU_CASES, ids=IDS)
def test_two_launches_of_50_give_the_figures_of_one_launch_of_100(case, monkeypatch):
    cfg = tj.config(case)
    o = tj.oracle_drift(case)
    one, kernel = _one_launch(case, monkeypatch)
    two, kernel2 = _hip_record(case, monkeypatch, chunks=(50, 50))
    assert kernel2 == kernel
    a = tj.drift(cfg, case['B'], o.acts, source=one, ref=o.ref)
    b = tj.drift(cfg, case['B'], o.acts, source=two, ref=o.ref)
    for name in ('d_obs', 'd_rew', 'd_shared', 'dp', 'dv', 'flips', 'contact'):       # every figure is a function of these
        assert np.array_equal(getattr(a, name), getattr(b, name)), name
    for x, y in zip(_worst(a), _worst(b)):
        assert np.array_equal(x, y)
    for k in ('pos', 'vel', 'landmarks', 'ep_step', 'ep_count'):
        assert np.array_equal(one['final_state'][k], two['final_state'][k]), k


# ------------------------------------------------------------------------------------------------ the B = 1 drop-in
def _dropin_records(N, seed, steps):
    """make_env (HIP, B = 1) and the Python float64 oracle env under one NumPy seed and the same actions (the pattern of
    tests/test_gpu_engine.py _drive_pair) -> (float32 record, float64 record) in the layout of tests/trajectory.py."""
    from multiagent_rl_amd import make_env
    np.random.seed(seed)
    gpu = make_env('simple_spread', n=N)
    np.random.seed(seed)
    ref = po.make_oracle_env('simple_spread', n=N)
    np.random.seed(seed)
    o_gpu = gpu.reset()
    np.random.seed(seed)
    o_ref = ref.reset()
    agents, lms = ref.world.agents, ref.world.landmarks

    def ref_state():
        return (np.stack([a.state.p_pos for a in agents])[None].copy(), np.stack([l.state.p_pos for l in lms])[None].copy())

    def ref_masks():
        return np.array([[sum(int(ref.scenario.is_collision(agents[j], agents[i])) << j for j in range(N)) for i in range(N)]],
                        np.uint64)
    pos0, lm0 = ref_state()
    src = dict(obs0=np.stack(o_gpu)[None], obs=[], rew=[], coll=[])
    want = dict(obs0=np.stack(o_ref)[None], pos0=pos0, obs=[], rew=[], coll=[], pos=[], lm_pre=[])
    rng = np.random.RandomState(1)
    for t in range(steps):
        acts = [np.eye(5)[i] for i in rng.randint(0, 5, N)]
        want['lm_pre'].append(ref_state()[1])
        o_gpu, r_gpu, d_gpu, i_gpu = gpu.step([a.copy() for a in acts])
        o_ref, r_ref, d_ref, i_ref = ref.step([a.copy() for a in acts])
        assert d_gpu == d_ref == [False] * N and i_gpu == i_ref == {'n': [{}] * N}          # exact integers
        assert all(isinstance(r, float) for r in r_gpu)
        for rec, o, r in ((src, o_gpu, r_gpu), (want, o_ref, r_ref)):
            assert all(x.dtype == np.float64 for x in o)
            rec['obs'].append(np.stack(o)[None])
            rec['rew'].append(np.array(r, np.float64)[None])
        src['coll'].append(_np(gpu.batched.reward()[1]).view(np.uint64))
        want['coll'].append(ref_masks())
        want['pos'].append(ref_state()[0])
    for rec in (src, want):
        for k in [k for k, v in rec.items() if isinstance(v, list)]:
            rec[k] = np.stack(rec[k])
        rec['final_obs'] = rec['obs']
        rec['rew_shared'] = rec['rew'].sum(-1)
        rec['done'] = np.zeros((steps, 1, N), np.uint8)
        rec['terminal'] = np.zeros((steps, 1), np.uint8)               # B = 1 drop-in: the caller ends episodes (run.py:50)
    return src, want


@pytest.mark.parametrize('N', [3, 6, 9, 12])
def test_dropin_under_the_reference_seed_protocol_against_the_float64_env(N):
    """np.random.seed(12345678 + cnt) as main.py:41-49 seeds run cnt: the reset draws float64 numbers, the HIP env starts from
    them rounded to float32 (start_rounded), then both run 25 steps on the same actions."""
    steps = 25
    cfg = co.make_config('simple_spread', N, max_episode_len=steps, auto_reset=False)
    worst = np.zeros(steps)
    flipped = 0
    for cnt in range(10):
        src, want = _dropin_records(N, 12345678 + cnt, steps)
        # the start: every coordinate within one float32 rounding of the float64 draw
        assert (np.abs(src['obs0'] - want['obs0'])[..., 2:4] <= tj._half_ulp32(want['obs0'][..., 2:4])).all()
        d = tj.compare(cfg, 1, src, want, start_rounded=True)
        flipped += tj.check_mask_flips(d)
        tj.check_rewards(d)
        tj.check_contact_free(d)
        worst = np.maximum(worst, d.d_obs[:, 0])
    tj.report(['# gpu (%s) drop-in make_env B=1 vs Python float64 env: simple_spread N=%d, seeds 12345678+0..9, %d mask bits flipped '
               'inside the drift band; worst |dobs| per step:' % (_device(), N, flipped),
               ' '.join('%.2e' % w for w in worst)])
