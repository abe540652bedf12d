"""World-constant sets away from the upstream defaults, shared by tests/test_oracle_world_constants.py (CPU: the C oracle
against the Python oracle at these constants) and tests/test_gpu_world_constants.py (GPU: every kernel form against the C
oracle at the same constants).  TEST INFRASTRUCTURE ONLY.

pw_config (include/pworld.h) and po_config (oracle/c_oracle.py) name their fields alike, so ONE function, ``apply_set``,
writes a set into either struct: the library's side and the oracle's side of a comparison cannot drift apart.  The Python
oracle is configured from the po_config itself (``configure_python_world``).

The values are chosen so that no product or quotient is exact and none is a power of two (the exception, contact_force =
64 in ``unit``, sits next to a dt, damping and size that are not): an error in operation order, or a reciprocal-multiply
where a division belongs, shows in the last bit.
"""
import numpy as np

from oracle import c_oracle as co

WORLD_FIELDS = ('dt', 'damping', 'contact_force', 'contact_margin', 'default_sensitivity', 'mass', 'landmark_size')

_STIFF = dict(dt=0.13, damping=0.1, contact_force=250.0, mass=0.7, contact_margin=2.5e-3)

SET_NAMES = ('canonical', 'heavy', 'stiff', 'unit', 'tag-roles', 'mixed')


def constant_set(name, scenario, N, A=0):
    """-> dict(world = {field: value} overrides, uses_accel, size / accel / max_speed = per-agent lists or None (canonical)).

    heavy      mass 3, action_force_uses_accel: the UNIT_MASS = false kernel instantiations, fscale = 3 (simple_tag: 9 / 12)
    stiff      contact_force 250 > 128: the general branch of collision_force_pair; a margin and (simple_spread) a size of
               their own: other host-derived thresholds
    unit       unit mass (the quad, trio and block-store forms need it) with a non-default sensitivity, fscale and dist_min
    tag-roles  simple_tag: stiff + per-role sizes, accelerations, a role WITHOUT a speed clamp, a landmark size of its own
    mixed      heterogeneous agents: only the generic kernel serves them
    """
    if isinstance(name, dict):                            # a set built by the caller (e.g. canonical with one size changed)
        return name
    tag = scenario == 'simple_tag'
    s = dict(world={}, uses_accel=False, size=None, accel=None, max_speed=None)
    if name == 'canonical':
        pass
    elif name == 'heavy':
        s.update(world=dict(dt=0.07, damping=0.4, contact_force=37.5, mass=3.0), uses_accel=True)
    elif name == 'stiff':
        s.update(world=dict(_STIFF))
        if not tag:
            s.update(size=[0.11] * N)
    elif name == 'unit':
        s.update(world=dict(dt=0.05, damping=0.3, contact_force=64.0, mass=1.0), uses_accel=True)
        if not tag:
            s.update(size=[0.11] * N, accel=[2.5] * N)
    elif name == 'tag-roles':
        assert tag and 0 < A < N
        s.update(world=dict(_STIFF, landmark_size=0.13),
                 size=[0.09 if i < A else 0.04 for i in range(N)],
                 accel=[2.5 if i < A else 4.5 for i in range(N)],
                 max_speed=[0.7 if i < A else -1.0 for i in range(N)])
    elif name == 'mixed':
        if tag:
            assert N - A >= 2
            s.update(size=[0.075 if i < A else 0.05 for i in range(N)])
            s['size'][A + 1] = 0.065                      # ONE good agent differs from its role
        else:
            assert N == 5
            s.update(size=[0.15, 0.1, 0.2, 0.12, 0.07], accel=[-1.0, 2.5, -1.0, 6.0, 3.0],
                     max_speed=[-1.0, 0.8, -1.0, 1.1, 0.5], uses_accel=True)
    else:
        raise ValueError(name)
    return s


def apply_set(cfg, s, overrides=None):
    """Writes a constant set into a pw_config or a po_config (same field names); ``overrides``: world fields written
    after the set (e.g. dt = 0)."""
    for k, v in list(s['world'].items()) + list((overrides or {}).items()):
        assert k in WORLD_FIELDS, k
        setattr(cfg, k, v)
    cfg.action_force_uses_accel = int(s['uses_accel'])
    for field, key in (('agent_size', 'size'), ('agent_accel', 'accel'), ('agent_max_speed', 'max_speed')):
        if s[key] is not None:
            assert len(s[key]) == cfg.num_agents
            for i, v in enumerate(s[key]):
                getattr(cfg, field)[i] = v
    return cfg


def oracle_config(name, scenario, N, L=None, A=0, overrides=None, **run):
    """po_config of one constant set.  ``run``: max_episode_len, auto_reset, seed, env_id_base."""
    cfg = co.make_config(scenario, N, num_landmarks=L, num_adversaries=A, **run)
    return apply_set(cfg, constant_set(name, scenario, N, A), overrides)


def both_configs(name, scenario, B, N, L=None, A=0, overrides=None, **run):
    """-> (pw_config for BatchedParticleEnv(config=...), po_config for COracle) holding the SAME constants."""
    from multiagent_rl_amd.env import make_config
    kw = dict(num_landmarks=L, **run)
    if scenario == 'simple_tag':
        kw.update(num_adversaries=A, num_good=N - A)
    else:
        kw.update(num_agents=N)
    pw = make_config(scenario, B, **kw)
    po = co.make_config(scenario, N, num_landmarks=L, num_adversaries=A, **run)
    s = constant_set(name, scenario, N, A)
    for cfg in (pw, po):
        apply_set(cfg, s, overrides)
    assert (pw.num_agents, pw.num_landmarks, pw.num_adversaries) == (po.num_agents, po.num_landmarks, po.num_adversaries)
    return pw, po


def configure_python_world(world, cfg):
    """oracle.particle_oracle World <- po_config: every world constant and every per-agent / per-landmark attribute."""
    world.dt, world.damping = cfg.dt, cfg.damping
    world.contact_force, world.contact_margin = cfg.contact_force, cfg.contact_margin
    world.action_force_uses_accel = bool(cfg.action_force_uses_accel)
    assert cfg.default_sensitivity == 5.0        # the Python oracle hard-codes it, as upstream does
    assert len(world.agents) == cfg.num_agents and len(world.landmarks) == cfg.num_landmarks
    for i, a in enumerate(world.agents):
        a.size = cfg.agent_size[i]
        a.accel = cfg.agent_accel[i] if cfg.agent_accel[i] >= 0 else None
        a.max_speed = cfg.agent_max_speed[i] if cfg.agent_max_speed[i] >= 0 else None
        a.initial_mass = cfg.mass
    for lm in world.landmarks:
        lm.size = cfg.landmark_size


def dist_min_f32(size_a, size_b):
    """dist_min as the float32 kernels and the float32 oracle form it: one float32 addition of the float32 sizes."""
    return np.float32(np.float32(size_a) + np.float32(size_b))
