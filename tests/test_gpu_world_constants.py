"""GPU parity away from the upstream world constants.

pw_config lets a caller change every world constant, and include/pworld.h promises the float32 oracle's bits whichever
kernel form runs.  tests/test_gpu_parity.py checks that at the upstream defaults; here every kernel form runs at the
constant sets of tests/world_constants.py (non-unit mass, the fork's force scale, a contact force beyond the fast branch of
collision_force_pair, other sizes / margins and so other host-derived thresholds, per-role simple_tag tables, heterogeneous
agents), and ``env.last_kernel()`` must name the instantiation the set is meant to reach.  The C oracle itself is anchored
at the same constants by tests/test_oracle_world_constants.py (CPU).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

from oracle import c_oracle as co  # noqa: E402  (checker only)
from tests import world_constants as wc  # noqa: E402
from tests.test_gpu_parity import AUTO, PATHS, KernelPath, _assert_same_bits, _coll, _np, _rand_state  # noqa: E402
from tests.test_gpu_parity import kernel_path  # noqa: E402,F401  (the fixture over all of PATHS)
from tests.test_gpu_policy_oracle import _assert_final_state, _replay_through_oracle  # noqa: E402

assert len(PATHS) == 21
FLT_MIN = float(np.finfo(np.float32).tiny)


def _mk(name, scenario, B, N, L=None, A=0, want_coll=True, dispatch=None, overrides=None, **run):
    """-> (BatchedParticleEnv, po_config): both built by tests/world_constants.both_configs from ONE constant set."""
    from multiagent_rl_amd.env import BatchedParticleEnv
    pw, po = wc.both_configs(name, scenario, B, N, L=L, A=A, overrides=overrides, **run)
    return BatchedParticleEnv(scenario, config=pw, want_coll=want_coll, dispatch=dispatch), po


def _self_bits(N):
    return (np.uint64(1) << np.arange(N, dtype=np.uint64))[None, :]


def _assert_kernel(env, path, cfg):
    """The kernel the dispatcher must have picked for this path and configuration (names: the PW_LAUNCH sites of
    csrc/pworld.hip).  With mass != 1 the name is asserted in full: these are the UNIT_MASS = false instantiations."""
    k = env.last_kernel()
    tag = cfg.scenario == co.SIMPLE_TAG
    N, L, A = cfg.num_agents, cfg.num_landmarks, cfg.num_adversaries
    um, d, wcoll = cfg.mass == 1.0, path.dispatch, path.want_coll
    if d.get('force_generic') or (tag and d.get('no_stream')):
        assert k.startswith('pw_rollout_kernel<'), k
        return
    if d.get('no_stream'):
        assert k == 'pw_spread_fast_kernel<%d>' % (N if N in (3, 6, 9, 12) else 0), k
        return
    if not tag and d.get('quad') == 1 and N == 6 and L == 6 and um:
        assert k.startswith('pw_spread_quad_kernel<true,true' if wcoll else 'pw_spread_quad_kernel<true'), k
        assert wcoll or not k.startswith('pw_spread_quad_kernel<true,true'), k
        return
    fam = ('pw_tag_' if tag else 'pw_spread_') + ('stream' if d.get('duo') == 0 else 'duo') + '_kernel'
    assert k.startswith(fam + '<'), (k, fam)                # mass != 1 under 'quad': fallen back to the duo form
    args = k[len(fam) + 1:-1].split(',')
    assert args[3 if tag else 2] == ('true' if um else 'false'), k
    if um:
        return
    if tag:
        roster = '0,-1,0' if wcoll else {(6, 4, 2): '6,4,2', (4, 3, 2): '4,3,2'}.get((N, A, L), '0,-1,0')
        # three waves where forced, else on grids of 512 .. 1280 workgroups (apply_dispatch's envs per wave: small batches
        # are spread over ~512 workgroups, '-dense' packs 64 // N envs)
        B = env.num_envs
        epw = min(d['envs_per_wave'], 64 // N) if d.get('envs_per_wave') else max(1, min({6: 8, 3: 16}.get(N, 64 // N), (B + 511) // 512))
        grid = (B + epw - 1) // epw
        trio = fam.startswith('pw_tag_duo') and (d['trio'] == 1 if 'trio' in d else 512 <= grid <= 1280)
        assert k == '%s<%s,false,%s%s>' % (fam, roster, 'true' if wcoll else 'false', ',true' if trio else ''), k
    else:
        key = N if N == L and not wcoll and N in (3, 6, 9, 12, 24, 48) else 0
        assert k == '%s<%d,%d,false%s>' % (fam, key, key, ',true' if wcoll else ''), k


# ---------------------------------------------------------------------------------------------- a. single step, every path
SPREAD = [dict(scenario='simple_spread', N=3, B=130), dict(scenario='simple_spread', N=6, B=257),
          dict(scenario='simple_spread', N=12, B=65), dict(scenario='simple_spread', N=5, L=2, B=77)]
TAG = [dict(scenario='simple_tag', N=6, A=4, B=123), dict(scenario='simple_tag', N=4, A=3, B=77)]
SINGLE = [(name, case) for name in ('heavy', 'stiff', 'unit') for case in SPREAD + TAG] + [
    ('tag-roles', dict(scenario='simple_tag', N=5, A=2, L=3, B=60))]


def _id(v):
    if isinstance(v, dict):
        return '%s-N%d-L%s-A%d-B%d' % (v['scenario'], v['N'], v.get('L'), v.get('A', 0), v['B'])
    return str(v)


@pytest.mark.parametrize('name,case', SINGLE, ids=_id)
def test_single_step_from_injected_states_at_other_constants(name, case, kernel_path):
    """tests/test_gpu_parity.py::test_single_step_from_injected_states, restated with a constant set: every output equals the
    float32 oracle bit for bit, the state is within 1e-5 of the float64 oracle, masks differ from it in at most 2 rows."""
    env, cfg = _mk(name, case['scenario'], case['B'], case['N'], L=case.get('L'), A=case.get('A', 0), max_episode_len=0,
                   want_coll=kernel_path.want_coll, dispatch=kernel_path.dispatch)
    B, N, L = env.num_envs, env.n, env.num_landmarks
    rng = np.random.RandomState(B * 131 + N)
    pos, vel, lm = _rand_state(rng, B, N, L)
    act = rng.randint(0, 5, (B, N)).astype(np.int32)
    env.set_state(pos, vel, lm)
    obs, rew, done, info = env.step(torch.from_numpy(act))
    st = env.get_state()
    _assert_kernel(env, kernel_path, cfg)
    o32 = co.COracle(cfg, B, np.float32)
    o32.set_state(pos, vel, lm)
    w = o32.step(act_idx=act)
    _assert_same_bits(_np(st['pos']), o32.pos, 'pos')
    _assert_same_bits(_np(st['vel']), o32.vel, 'vel')
    _assert_same_bits(_np(st['landmarks']), o32.lm, 'landmarks')
    _assert_same_bits(_np(obs), w['obs'], 'obs')
    _assert_same_bits(_np(rew), w['rew'], 'rew')
    if 'coll' in info:
        _assert_same_bits(_coll(info['coll']), w['coll'], 'coll')
    assert ('coll' in info) == kernel_path.want_coll
    _assert_same_bits(_np(done).astype(np.uint8), w['done'], 'done')
    _assert_same_bits(_np(info['terminal']).astype(np.uint8), w['terminal'], 'terminal')
    assert not _np(done).any()
    _assert_same_bits(_np(info['rew_shared']), w['rew_shared'], 'rew_shared')
    o64 = co.COracle(cfg, B, np.float64)
    o64.set_state(pos, vel, lm)
    w64 = o64.step(act_idx=act)
    np.testing.assert_allclose(_np(st['pos']), o64.pos, rtol=0, atol=1e-5)
    np.testing.assert_allclose(_np(st['vel']), o64.vel, rtol=0, atol=1e-5)
    np.testing.assert_allclose(_np(obs), w64['obs'], rtol=0, atol=1e-5)
    diff = (_coll(info['coll']) if 'coll' in info else w['coll']) ^ w64['coll']
    assert np.count_nonzero(diff) <= 2, 'collision masks differ from the float64 oracle in %d rows' % np.count_nonzero(diff)
    assert (w['coll'] != _self_bits(N)).any()              # the crowded half of the batch really has contacts


# ---------------------------------------------------------------------------------------------- b. rollout, two auto-resets
ROLL_PATHS = ['duo', 'stream', 'duo+coll', 'trio', 'trio+block', 'duo+block-dense', 'fast', 'generic']


ROLLS = [(name, case, path) for name in ('heavy', 'stiff', 'unit') for case in (SPREAD[1], TAG[0])
         for path in ROLL_PATHS + (['quad'] if name == 'unit' else [])]     # the quad form needs unit mass


@pytest.mark.parametrize('name,case,path', ROLLS, ids=_id)
def test_rollout_across_two_auto_resets_at_other_constants(name, case, path):
    path = KernelPath(path)
    T, ep_len = 58, 25
    env, cfg = _mk(name, case['scenario'], case['B'], case['N'], A=case.get('A', 0), max_episode_len=ep_len, auto_reset=True,
                   seed=99, env_id_base=1 << 33, want_coll=path.want_coll, dispatch=path.dispatch)
    B, N = env.num_envs, env.n
    acts = np.random.RandomState(5).randint(0, 5, (T, B, N)).astype(np.int32)
    o32 = co.COracle(cfg, B, np.float32)
    _assert_same_bits(_np(env.reset()), o32.reset(), 'reset obs')
    out = env.rollout(torch.from_numpy(acts))
    _assert_kernel(env, path, cfg)
    resets = hits = 0
    for t in range(T):
        w = o32.step(act_idx=acts[t])
        _assert_same_bits(_np(out['obs'][t]), w['obs'], 'obs[%d]' % t)
        _assert_same_bits(_np(out['rew'][t]), w['rew'], 'rew[%d]' % t)
        _assert_same_bits(_np(out['rew_shared'][t]), w['rew_shared'], 'rew_shared[%d]' % t)
        _assert_same_bits(_np(out['terminal'][t]).astype(np.uint8), w['terminal'], 'terminal[%d]' % t)
        if 'coll' in out:
            _assert_same_bits(_coll(out['coll'][t]), w['coll'], 'coll[%d]' % t)
        hits += int((w['coll'] != _self_bits(N)).sum())
        if w['terminal'].any():
            resets += 1
            _assert_same_bits(_np(out['final_obs'][t]), w['final_obs'], 'final_obs[%d]' % t)
            assert w['terminal'].all() and (t + 1) % ep_len == 0
    assert resets == T // ep_len and hits > 0
    _assert_final_state(env, o32)


# ---------------------------------------------------------------------------------------------- c. the collision threshold
PAIR_CENTRES = np.array([[-1.2, -0.8], [1.2, -0.8], [0.0, 1.0]])        # > 2.1 apart: only the constructed pairs interact


def _place_pairs(rng, B, pairs, radius):
    """[B, N, 2] float32 positions: agent ``a`` of pair k = (a, b) near PAIR_CENTRES[k], its partner ``b`` at distance
    radius[:, k] from it at a random angle -- one eighth of the pairs exactly on the x axis (dy == 0: the numerator of the y
    force is an exact zero).  ``pairs`` [B, K, 2] agent indices, ``radius`` [B, K] float64.  Computed in float64, rounded to
    float32 once."""
    K = pairs.shape[1]
    N = int(pairs.max()) + 1
    pos = np.zeros((B, N, 2))
    base = PAIR_CENTRES[None, :K] + rng.uniform(-0.05, 0.05, (B, K, 2))
    ang = rng.uniform(0, 2 * np.pi, (B, K))
    on_axis = rng.randint(0, 8, (B, K)) == 0
    ang[on_axis] = np.pi * rng.randint(0, 2, int(on_axis.sum()))
    off = radius[..., None] * np.stack([np.cos(ang), np.sin(ang)], -1)
    off[on_axis, 1] = 0.0
    e = np.arange(B)[:, None]
    pos[e, pairs[..., 0]] = base
    pos[e, pairs[..., 1]] = base + off
    return pos.astype(np.float32), on_axis


def _pair_bits(coll, pairs):
    """is_collision(a, b) of every constructed pair, from the [B, N] uint64 masks."""
    e = np.arange(coll.shape[0])[:, None]
    return ((coll[e, pairs[..., 0]] >> pairs[..., 1].astype(np.uint64)) & np.uint64(1)).astype(bool)


THRESHOLD_PATHS = ['duo+coll', 'stream+coll', 'quad+coll', 'fast', 'generic']


def _threshold_inputs(size, B=512):
    rng = np.random.RandomState(int(size * 1e4))
    pairs = np.tile(np.array([[0, 1], [2, 3], [4, 5]]), (B, 1, 1))
    dmin = float(wc.dist_min_f32(size, size))
    radius = dmin * (1.0 + rng.uniform(-3, 3, (B, 3)) * 2.0 ** -24)
    pos, on_axis = _place_pairs(rng, B, pairs, radius)
    vel = rng.uniform(-1.5, 1.5, (B, 6, 2)).astype(np.float32)
    lm = rng.uniform(-0.9, 0.9, (B, 6, 2)).astype(np.float32)
    act = rng.randint(0, 5, (B, 6)).astype(np.int32)
    return pairs, pos, vel, lm, act, on_axis


@pytest.mark.parametrize('path', THRESHOLD_PATHS)
@pytest.mark.parametrize('size', [0.15, 0.11, 0.0625, 0.1, 0.2])
def test_collision_threshold_with_the_clock_stopped(size, path):
    """dt = 0: a step leaves the positions exactly where the test put them, so the post-step collision test runs on pairs
    placed within +-3 * 2^-24 (relative) of dist_min = size + size -- the host-derived coll_thr2 of this size decides every one
    of them.  Masks and rewards equal the float32 oracle bit for bit."""
    path = KernelPath(path)
    B, N = 512, 6
    s = dict(wc.constant_set('canonical', 'simple_spread', N), size=[size] * N)
    env, cfg = _mk(s, 'simple_spread', B, N, overrides=dict(dt=0.0), max_episode_len=0, want_coll=True, dispatch=path.dispatch)
    pairs, pos, vel, lm, act, on_axis = _threshold_inputs(size, B)
    o32 = co.COracle(cfg, B, np.float32)
    o32.set_state(pos, vel, lm)
    w = o32.step(act_idx=act)
    # conditions on the INPUTS, judged on the oracle's output: the clock is stopped, and the pairs straddle the threshold
    assert np.array_equal(o32.pos, pos)
    hit = _pair_bits(w['coll'], pairs)
    assert 0.25 <= hit.mean() <= 0.60, hit.mean()
    assert on_axis.sum() >= B // 4 and 0 < hit[on_axis].sum() < on_axis.sum()
    off = w['coll'] & ~_self_bits(N)
    assert sum(int(((off >> np.uint64(j)) & np.uint64(1)).sum()) for j in range(N)) == 2 * hit.sum()   # nobody else touches
    env.set_state(pos, vel, lm)
    obs, rew, done, info = env.step(torch.from_numpy(act))
    _assert_kernel(env, path, cfg)
    _assert_same_bits(_coll(info['coll']), w['coll'], 'coll')
    _assert_same_bits(_np(rew), w['rew'], 'rew')
    _assert_same_bits(_np(env.get_state()['pos']), pos, 'pos')


def _tag_pairs(B):
    """simple_tag 4 + 2: one pair per class combination -- even envs (adv, adv), (adv, good), (adv, good); odd envs (adv, adv),
    (adv, adv), (good, good)."""
    pairs = np.empty((B, 3, 2), np.int64)
    pairs[0::2] = [[0, 1], [2, 4], [3, 5]]
    pairs[1::2] = [[0, 1], [2, 3], [4, 5]]
    return pairs


@pytest.mark.parametrize('path', THRESHOLD_PATHS)
def test_tag_role_thresholds_with_the_clock_stopped(path):
    """The same construction for simple_tag 4 + 2 with per-role sizes (0.09 / 0.04): every entry of the 2 x 2 class table of
    collision thresholds decides pairs placed on it."""
    path = KernelPath(path)
    B, N, A = 512, 6, 4
    env, cfg = _mk('tag-roles', 'simple_tag', B, N, A=A, overrides=dict(dt=0.0), max_episode_len=0, want_coll=True,
                   dispatch=path.dispatch)
    rng = np.random.RandomState(17)
    pairs = _tag_pairs(B)
    size = np.array([cfg.agent_size[i] for i in range(N)])
    dmin = wc.dist_min_f32(size[pairs[..., 0]], size[pairs[..., 1]]).astype(np.float64)
    pos, on_axis = _place_pairs(rng, B, pairs, dmin * (1.0 + rng.uniform(-3, 3, (B, 3)) * 2.0 ** -24))
    vel = rng.uniform(-1.5, 1.5, (B, N, 2)).astype(np.float32)
    lm = (np.array([[-0.3, 0.0], [0.3, 0.0]]) + rng.uniform(-0.02, 0.02, (B, 2, 2))).astype(np.float32)
    act = rng.randint(0, 5, (B, N)).astype(np.int32)
    o32 = co.COracle(cfg, B, np.float32)
    o32.set_state(pos, vel, lm)
    w = o32.step(act_idx=act)
    assert np.array_equal(o32.pos, pos)
    hit = _pair_bits(w['coll'], pairs)
    cls = (pairs[..., 0] >= A).astype(int) + (pairs[..., 1] >= A).astype(int)     # 0: adv-adv, 1: adv-good, 2: good-good
    for c in range(3):
        assert 0.25 <= hit[cls == c].mean() <= 0.60, (c, hit[cls == c].mean())
    env.set_state(pos, vel, lm)
    obs, rew, done, info = env.step(torch.from_numpy(act))
    _assert_kernel(env, path, cfg)
    _assert_same_bits(_coll(info['coll']), w['coll'], 'coll')
    _assert_same_bits(_np(rew), w['rew'], 'rew')
    assert (np.abs(w['rew']) >= 10).any()


# ---------------------------------------------------------------------------------------------- d. the far cut
FAR_PATHS = ['duo', 'stream', 'quad', 'fast', 'generic', 'trio', 'trio+block']


def _zero_and_subnormal(vel):
    """Fractions of agents whose velocity is exactly zero / nonzero with every component below FLT_MIN."""
    mag = np.abs(vel.astype(np.float64)).max(-1)
    return float((mag == 0).mean()), float(((mag > 0) & (mag < FLT_MIN)).mean())


@pytest.mark.parametrize('path', FAR_PATHS)
@pytest.mark.parametrize('name', ['canonical', 'heavy', 'stiff'])
def test_far_cut_where_forces_are_subnormal(name, path):
    """Pairs at dist_min + s * contact_margin, s in [84, 90], at rest, no action: beyond pw_exp's exact-zero cut (s > 87) the
    contact force is exactly zero, below it a subnormal or barely normal number.  A kernel that flushes denormals, or that
    skips a pair as "provably far" a hair too early, gives other bits here -- and nowhere else in the suite."""
    path = KernelPath(path)
    B, N = 256, 6
    env, cfg = _mk(name, 'simple_spread', B, N, max_episode_len=0, want_coll=path.want_coll, dispatch=path.dispatch)
    rng = np.random.RandomState(23)
    pairs = np.tile(np.array([[0, 1], [2, 3], [4, 5]]), (B, 1, 1))
    dmin = float(wc.dist_min_f32(cfg.agent_size[0], cfg.agent_size[0]))
    pos, _ = _place_pairs(rng, B, pairs, dmin + rng.uniform(84, 90, (B, 3)) * cfg.contact_margin)
    vel = np.zeros((B, N, 2), np.float32)
    lm = rng.uniform(-0.9, 0.9, (B, N, 2)).astype(np.float32)
    act = np.zeros((B, N), np.int32)
    o32 = co.COracle(cfg, B, np.float32)
    o32.set_state(pos, vel, lm)
    o32.step(act_idx=act)
    zero, sub = _zero_and_subnormal(o32.vel)               # conditions on the inputs, judged on the oracle's output
    assert zero >= 0.25 and sub >= 0.25, (zero, sub)
    env.set_state(pos, vel, lm)
    env.step(torch.from_numpy(act))
    _assert_kernel(env, path, cfg)
    st = env.get_state()
    _assert_same_bits(_np(st['vel']), o32.vel, 'vel')
    _assert_same_bits(_np(st['pos']), o32.pos, 'pos')


@pytest.mark.parametrize('path', ['duo', 'stream', 'trio', 'generic'])
def test_tag_landmark_far_cut_per_role(path):
    """simple_tag with per-role sizes and a landmark size of its own: one adversary and one good agent each sit in the
    near-cut band of a landmark (dist_min_lm of their class + s * contact_margin), everybody else far from everything --
    landmarks do not enter the collision masks, so this is where the per-class landmark thresholds are decided."""
    path = KernelPath(path)
    B, N, A = 256, 6, 4
    env, cfg = _mk('tag-roles', 'simple_tag', B, N, A=A, max_episode_len=0, want_coll=path.want_coll, dispatch=path.dispatch)
    rng = np.random.RandomState(29)
    lm = (np.array([[-0.7, 0.0], [0.7, 0.0]]) + rng.uniform(-0.03, 0.03, (B, 2, 2))).astype(np.float32)
    far = np.array([[-0.7, 1.3], [0.0, 1.3], [0.7, 1.3], [0.0, -1.3]])
    pos = np.zeros((B, N, 2))
    pos[:, [1, 2, 3, 5]] = far[None] + rng.uniform(-0.03, 0.03, (B, 4, 2))
    for agent, l in ((0, 0), (4, 1)):
        r = float(wc.dist_min_f32(cfg.agent_size[agent], cfg.landmark_size)) + rng.uniform(84, 90, B) * cfg.contact_margin
        ang = rng.uniform(0, 2 * np.pi, B)
        pos[:, agent] = lm[:, l].astype(np.float64) + r[:, None] * np.stack([np.cos(ang), np.sin(ang)], -1)
    pos = pos.astype(np.float32)
    vel = np.zeros((B, N, 2), np.float32)
    act = np.zeros((B, N), np.int32)
    o32 = co.COracle(cfg, B, np.float32)
    o32.set_state(pos, vel, lm)
    o32.step(act_idx=act)
    assert not o32.vel[:, [1, 2, 3, 5]].any()
    for agent in (0, 4):                                    # each class: some beyond the cut, some subnormal
        zero, sub = _zero_and_subnormal(o32.vel[:, agent])
        assert zero >= 0.25 and sub >= 0.25, (agent, zero, sub)
    env.set_state(pos, vel, lm)
    env.step(torch.from_numpy(act))
    _assert_kernel(env, path, cfg)
    st = env.get_state()
    _assert_same_bits(_np(st['vel']), o32.vel, 'vel')
    _assert_same_bits(_np(st['pos']), o32.pos, 'pos')


# ---------------------------------------------------------------------------------------------- e. one-launch policy rollouts
POLICY_FORM = dict(v3=(3, 'pw_policy_rollout3_kernel'), v3j=(4, 'pw_policy_rollout3j_kernel'))


@pytest.mark.parametrize('form,N,B,name', [
    ('v3', 6, 100, 'heavy'), ('v3', 6, 100, 'unit'),
    ('v3j', 6, 100, 'heavy'), ('v3j', 6, 100, 'unit'), ('v3j', 6, 100, 'stiff'),
    ('v3j', 16, 33, 'heavy'), ('v3j', 16, 33, 'unit'), ('v3j', 16, 33, 'stiff')])
def test_spread_policy_rollout_at_other_constants_equals_the_oracle_on_its_own_actions(form, N, B, name):
    """Forms 3 and 3j carry their own copy of the step and read mass, fscale, dt, damp, contact_force from the same parameter
    blocks: the launch's own sampled actions replayed through the oracle reproduce every environment output and the final
    state, 27 steps across a reset."""
    from multiagent_rl_amd.policy import ActorNetwork, FusedActor
    torch.manual_seed(4)
    T = 27
    env, cfg = _mk(name, 'simple_spread', B, N, max_episode_len=25, auto_reset=True, seed=21, want_coll=False)
    env.set_dispatch(policy_form=POLICY_FORM[form][0])
    o32 = co.COracle(cfg, B, np.float32)
    actor = FusedActor(ActorNetwork(env.obs_dim, 5).cuda().eval(), seed=9)
    _assert_same_bits(_np(env.reset()), o32.reset(), 'reset obs')
    got = actor.rollout(env, T)
    assert env.last_kernel() == POLICY_FORM[form][1], env.last_kernel()
    assert len(np.unique(_np(got['act']))) == 5
    assert _replay_through_oracle(o32, got, T) == 1
    _assert_final_state(env, o32)


@pytest.mark.parametrize('name,A,G,L', [('heavy', 4, 2, None), ('tag-roles', 2, 3, 3)], ids=['heavy-4+2', 'tag-roles-2+3'])
def test_tag_policy_rollout_at_other_constants_equals_the_oracle_on_its_own_actions(name, A, G, L):
    from multiagent_rl_amd.policy import ActorNetwork, FusedActor
    torch.manual_seed(5)
    B, T = 37, 30
    env, cfg = _mk(name, 'simple_tag', B, A + G, L=L, A=A, max_episode_len=25, auto_reset=True, seed=31, want_coll=False)
    o32 = co.COracle(cfg, B, np.float32)
    actor = FusedActor(ActorNetwork(env.obs_dim, 5).cuda().eval(), seed=9)
    _assert_same_bits(_np(env.reset()), o32.reset(), 'reset obs')
    got = actor.rollout(env, T)
    assert 'policy_rollout_tag' in env.last_kernel(), env.last_kernel()
    assert len(np.unique(_np(got['act']))) == 5
    assert _replay_through_oracle(o32, got, T) == 1
    assert float(got['rew'].abs().sum()) > 0
    _assert_final_state(env, o32)


# ---------------------------------------------------------------------------------------------- f. heterogeneous agents
@pytest.mark.parametrize('case', [dict(scenario='simple_spread', N=5, B=77), dict(scenario='simple_tag', N=5, A=2, B=77)], ids=_id)
def test_heterogeneous_agents_fall_back_to_the_generic_kernel(case):
    """Per-agent sizes / accelerations / speed clamps (simple_tag: one good agent unlike its role) are served by
    pw_rollout_kernel alone under the default dispatch -- one step and a 30-step auto-reset rollout equal the oracle bit
    for bit -- and the one-launch policy rollout refuses the handle."""
    from multiagent_rl_amd._lib import PworldError
    from multiagent_rl_amd.policy import ActorNetwork, FusedActor
    kw = dict(L=case.get('L'), A=case.get('A', 0), dispatch=dict(AUTO))
    env, cfg = _mk('mixed', case['scenario'], case['B'], case['N'], max_episode_len=0, **kw)
    B, N, L = env.num_envs, env.n, env.num_landmarks
    rng = np.random.RandomState(B * 131 + N)
    pos, vel, lm = _rand_state(rng, B, N, L)
    act = rng.randint(0, 5, (B, N)).astype(np.int32)
    env.set_state(pos, vel, lm)
    obs, rew, done, info = env.step(torch.from_numpy(act))
    assert env.last_kernel().startswith('pw_rollout_kernel'), env.last_kernel()
    o32 = co.COracle(cfg, B, np.float32)
    o32.set_state(pos, vel, lm)
    w = o32.step(act_idx=act)
    for got, key in ((obs, 'obs'), (rew, 'rew'), (info['rew_shared'], 'rew_shared')):
        _assert_same_bits(_np(got), w[key], key)
    _assert_same_bits(_coll(info['coll']), w['coll'], 'coll')
    assert (w['coll'] != _self_bits(N)).any()
    st = env.get_state()
    _assert_same_bits(_np(st['pos']), o32.pos, 'pos')
    _assert_same_bits(_np(st['vel']), o32.vel, 'vel')
    # 30 steps across an auto-reset
    T = 30
    env, cfg = _mk('mixed', case['scenario'], case['B'], case['N'], max_episode_len=25, auto_reset=True, seed=13, **kw)
    acts = rng.randint(0, 5, (T, B, N)).astype(np.int32)
    o32 = co.COracle(cfg, B, np.float32)
    _assert_same_bits(_np(env.reset()), o32.reset(), 'reset obs')
    out = env.rollout(torch.from_numpy(acts))
    assert env.last_kernel().startswith('pw_rollout_kernel'), env.last_kernel()
    for t in range(T):
        w = o32.step(act_idx=acts[t])
        for key in ('obs', 'rew', 'rew_shared'):
            _assert_same_bits(_np(out[key][t]), w[key], '%s[%d]' % (key, t))
        _assert_same_bits(_coll(out['coll'][t]), w['coll'], 'coll[%d]' % t)
        _assert_same_bits(_np(out['terminal'][t]).astype(np.uint8), w['terminal'], 'terminal[%d]' % t)
        if w['terminal'].any():
            assert t == 24
            _assert_same_bits(_np(out['final_obs'][t]), w['final_obs'], 'final_obs[%d]' % t)
    _assert_final_state(env, o32)
    torch.manual_seed(1)
    actor = FusedActor(ActorNetwork(env.obs_dim, 5).cuda().eval(), seed=9)
    with pytest.raises(PworldError, match='libpworld error -1'):      # PW_EINVAL
        actor.rollout(env, 2)


# ---------------------------------------------------------------------------------------------- communication scenarios
COMM_WORLD = dict(dt=0.07, damping=0.4, mass=3.0, default_sensitivity=3.5)


@pytest.mark.parametrize('scenario', ['simple_reference', 'simple_speaker_listener'])
def test_communication_scenarios_at_other_world_constants(scenario):
    """What the communication scenarios leave free -- dt, damping, mass, default_sensitivity -- against CRefOracle(float32):
    pw_rollout over 30 steps across a reset, and for simple_reference the one-launch policy rollout, bit for bit."""
    from multiagent_rl_amd.policy import ActorNetwork, FusedActor
    B, T = 100, 30
    s = dict(wc.constant_set('canonical', scenario, 2), world=dict(COMM_WORLD))
    run = dict(max_episode_len=25, auto_reset=True, seed=77, want_coll=False)
    env, cfg = _mk(s, scenario, B, 2, **run)
    assert (cfg.dt, cfg.mass, cfg.default_sensitivity) == (0.07, 3.0, 3.5)
    o32 = co.CRefOracle(cfg, B, np.float32)
    _assert_same_bits(_np(env.reset()), o32.reset(), 'reset obs')
    rng = np.random.RandomState(4)
    ref = scenario == 'simple_reference'
    acts = np.stack([rng.randint(0, 5, (T, B, 2)), rng.randint(0, 10, (T, B, 2))] if ref else
                    [rng.randint(0, 3, (T, B)), rng.randint(0, 5, (T, B))], -1).astype(np.int32)
    out = env.rollout(torch.from_numpy(acts))
    assert env.last_kernel().startswith('pw_reference_rollout_kernel'), env.last_kernel()
    resets = 0
    for t in range(T):
        w = o32.step(act_idx=acts[t][..., 0], act_comm=acts[t][..., 1]) if ref else o32.step(act_idx=acts[t])
        _assert_same_bits(_np(out['obs'][t]), w['obs'], 'obs[%d]' % t)
        _assert_same_bits(_np(out['rew'][t]), w['rew'], 'rew[%d]' % t)
        _assert_same_bits(_np(out['rew_shared'][t]), (np.float32(0) + w['rew'][:, 0]) + w['rew'][:, 1], 'rew_shared[%d]' % t)
        _assert_same_bits(_np(out['terminal'][t]).astype(np.uint8), w['terminal'], 'terminal[%d]' % t)
        if w['terminal'].any():
            resets += 1
            _assert_same_bits(_np(out['final_obs'][t]), w['final_obs'], 'final_obs[%d]' % t)
    assert resets == 1
    _assert_final_state(env, o32, extra=('comm', 'goal'))
    if not ref:
        return
    torch.manual_seed(6)
    env, cfg = _mk(s, scenario, B, 2, **dict(run, seed=17))
    o32 = co.CRefOracle(cfg, B, np.float32)
    actor = FusedActor(ActorNetwork(env.obs_dim, [5, 10]).cuda().eval(), seed=9)
    _assert_same_bits(_np(env.reset()), o32.reset(), 'reset obs')
    got = actor.rollout(env, T)
    assert 'policy_rollout_ref' in env.last_kernel(), env.last_kernel()
    a = _np(got['act'])
    assert a.shape == (T, B, 2, 2) and a[..., 0].max() <= 4 and 4 < a[..., 1].max() <= 9
    assert _replay_through_oracle(o32, got, T, two_head=True) == 1
    _assert_final_state(env, o32, extra=('comm', 'goal'))
