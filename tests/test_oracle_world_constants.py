"""CPU: the C oracle away from the upstream world constants.

tests/test_gpu_world_constants.py compares every kernel form with ``COracle(float32)`` at the constant sets of
tests/world_constants.py.  That is only worth something if the C oracle is right THERE, so for every set and shape the GPU
tests use:

* ``COracle(float64)`` against the Python oracle (oracle/particle_oracle.py, the restatement of upstream's loops) configured
  the same way -- dt, damping, contact_force, contact_margin, the fork knob, per-agent size / accel / max_speed / mass, landmark
  size -- one step from crowded injected states: positions, velocities, observation rows and rewards are EQUAL (both are IEEE
  float64 in the same operation order; measured difference 0.0 -- but for simple_tag's exp() boundary penalty, where the C
  library's exp and NumPy's may round differently);
* ``COracle(float32)`` against ``COracle(float64)``, one step from the states the GPU single-step test injects: the state and the
  rows within the project's 1e-5 bar, collision masks different in at most 2 rows -- the conditions the GPU test then asserts of
  the kernels hold of the reference alone.
"""
import numpy as np
import pytest

from oracle import c_oracle as co
from oracle import particle_oracle as po
from tests import world_constants as wc
from tests.test_gpu_parity import _rand_state

SPREAD = [dict(scenario='simple_spread', N=3, B=130), dict(scenario='simple_spread', N=6, B=257),
          dict(scenario='simple_spread', N=12, B=65), dict(scenario='simple_spread', N=5, L=2, B=77)]
TAG = [dict(scenario='simple_tag', N=6, A=4, B=123), dict(scenario='simple_tag', N=4, A=3, B=77)]

# (constant set, shape): exactly what test_gpu_world_constants.py steps, per-agent arrays included
CONFIGS = [(name, case) for name in ('heavy', 'stiff', 'unit') for case in SPREAD + TAG] + [
    ('tag-roles', dict(scenario='simple_tag', N=5, A=2, L=3, B=60)),
    ('mixed', dict(scenario='simple_spread', N=5, B=77)),
    ('mixed', dict(scenario='simple_tag', N=5, A=2, B=77)),
    ('canonical', dict(scenario='simple_spread', N=6, B=257)),
]
IDS = ['%s-%s-N%d-L%s-A%d' % (n, c['scenario'], c['N'], c.get('L'), c.get('A', 0)) for n, c in CONFIGS]


def _cfg(name, case, **run):
    return wc.oracle_config(name, case['scenario'], case['N'], L=case.get('L'), A=case.get('A', 0), **run)


def _python_env(cfg):
    if cfg.scenario == co.SIMPLE_TAG:
        env = po.make_oracle_env('simple_tag', num_adversaries=cfg.num_adversaries,
                                 num_good=cfg.num_agents - cfg.num_adversaries, num_landmarks=cfg.num_landmarks)
    else:
        env = po.make_oracle_env('simple_spread', n=cfg.num_agents, num_landmarks=cfg.num_landmarks)
    wc.configure_python_world(env.world, cfg)
    return env


@pytest.mark.parametrize('name,case', CONFIGS, ids=IDS)
def test_c_float64_oracle_equals_python_oracle_at_these_constants(name, case):
    cfg = _cfg(name, case, max_episode_len=0)
    B, N, L = 30, cfg.num_agents, cfg.num_landmarks
    rng = np.random.RandomState(1000 + 7 * N + len(name))
    pos, vel, lm = [x.astype(np.float64) for x in _rand_state(rng, B, N, L)]
    pos[:B // 2] *= 0.6                                       # crowd the first half further: several contacts per env
    act = rng.randint(0, 5, (B, N))
    o64 = co.COracle(cfg, B, np.float64)
    o64.set_state(pos, vel, lm)
    w = o64.step(act_idx=act)
    D = o64.D
    clamped = boundary = 0
    for e in range(B):
        env = _python_env(cfg)
        po.set_world_state(env.world, pos[e], vel[e], lm[e])
        obs, rew, done, _ = env.step([po.onehot(a) for a in act[e]])
        p, v, _ = po.get_world_state(env.world)
        rows = np.stack([np.pad(x, (0, D - len(x))) for x in obs])
        assert np.array_equal(o64.pos[e], p), (e, np.abs(o64.pos[e] - p).max())
        assert np.array_equal(o64.vel[e], v), (e, np.abs(o64.vel[e] - v).max())
        assert np.array_equal(w['obs'][e], rows), (e, np.abs(w['obs'][e] - rows).max())
        rew = np.array(rew, np.float64)
        # simple_tag's boundary penalty of a good agent beyond |x| = 1 is exp(2x - 2): the C library's exp and NumPy's are two
        # implementations, each within 1 ulp of the true value (seen: 1 ulp apart in 5 of these 660 environments, only there).
        # Two penalties <= 10 (ulp 2^-49), 2 ulp apart each, then two subtractions from |r| < 64 (ulp 2^-47) on perturbed
        # operands: 4 * 2^-49 + 2 * 2^-47 < 3e-14.  Every other reward is EQUAL.
        loose = np.zeros(N, bool)
        if cfg.scenario == co.SIMPLE_TAG:
            loose[cfg.num_adversaries:] = (np.abs(p[cfg.num_adversaries:]) >= 1.0).any(axis=1)
        assert np.array_equal(w['rew'][e][~loose], rew[~loose]), (e, w['rew'][e], rew)
        np.testing.assert_allclose(w['rew'][e][loose], rew[loose], rtol=0, atol=3e-14)
        boundary += int(loose.sum())
        for i, a in enumerate(env.world.agents):
            if a.max_speed is not None:
                clamped += int(abs(np.hypot(*v[i]) - a.max_speed) < 1e-12)
    contacts = int((w['coll'] & ~(np.uint64(1) << np.arange(N, dtype=np.uint64))[None, :]).astype(bool).sum())
    assert contacts >= 4                                      # the crowded half really has contacts
    if any(cfg.agent_max_speed[i] >= 0 for i in range(N)):
        assert clamped >= 4                                   # ... and the speed clamp really acted
    if cfg.scenario == co.SIMPLE_TAG:
        assert boundary >= 4                                  # ... and good agents beyond |x| = 1 were seen


@pytest.mark.parametrize('name,case', CONFIGS, ids=IDS)
def test_c_float32_oracle_within_1e5_of_float64_at_these_constants(name, case):
    cfg = _cfg(name, case, max_episode_len=0)
    B, N, L = case['B'], cfg.num_agents, cfg.num_landmarks
    rng = np.random.RandomState(B * 131 + N)                  # the states test_gpu_world_constants.py injects
    pos, vel, lm = _rand_state(rng, B, N, L)
    act = rng.randint(0, 5, (B, N)).astype(np.int32)
    o32, o64 = co.COracle(cfg, B, np.float32), co.COracle(cfg, B, np.float64)
    o32.set_state(pos, vel, lm)
    o64.set_state(pos, vel, lm)
    w32, w64 = o32.step(act_idx=act), o64.step(act_idx=act)
    np.testing.assert_allclose(o32.pos, o64.pos, rtol=0, atol=1e-5)
    np.testing.assert_allclose(o32.vel, o64.vel, rtol=0, atol=1e-5)
    np.testing.assert_allclose(w32['obs'], w64['obs'], rtol=0, atol=1e-5)
    rows = np.count_nonzero(w32['coll'] ^ w64['coll'])
    assert rows <= 2, 'collision masks of the float32 and float64 oracle differ in %d rows' % rows
    assert (w32['coll'] != (np.uint64(1) << np.arange(N, dtype=np.uint64))[None, :]).any()


def test_clock_stopped_step_leaves_positions_exactly_in_place():
    """dt = 0: what the GPU collision-threshold test relies on -- the post-step collision test runs on the positions the
    test chose, whatever the velocities and actions."""
    cfg = wc.oracle_config('canonical', 'simple_spread', 6, overrides=dict(dt=0.0), max_episode_len=0)
    rng = np.random.RandomState(4)
    pos, vel, lm = _rand_state(rng, 64, 6, 6)
    for dtype in (np.float32, np.float64):
        o = co.COracle(cfg, 64, dtype)
        o.set_state(pos, vel, lm)
        o.step(act_idx=rng.randint(0, 5, (64, 6)))
        assert np.array_equal(o.pos, pos.astype(dtype))
        assert not np.array_equal(o.vel, vel.astype(dtype))
