"""Free-running float32 trajectories against the float64 C oracle -- TEST INFRASTRUCTURE (imports ``oracle`` only).

``drift(cfg, B, acts, source=None)`` steps a float32 source and the float64 oracle through ``T = len(acts)`` steps on the same
int32 actions from the same Philox reset and returns a ``Drift``: per step and env the differences of observations, rewards,
shared rewards, positions and velocities, the collision-mask flips, and which envs have had a contact so far in their episode.
The source is the float32 C oracle (``source=None``) or recorded outputs of the HIP env (a dict of ``[T, ...]`` arrays: obs,
final_obs, rew, rew_shared, done, terminal, optionally coll, plus ``obs0`` = the reset observation).  simple_reference and
simple_speaker_listener go through ``CRefOracle``.  On terminal steps the pre-reset ``final_obs`` is what is compared.

``check_structure(d)`` asserts what follows from the construction alone (no drift figure is typed in anywhere):
reset states equal, clocks identical, mask flips only inside the drift band, rewards inside their Lipschitz bound, contact-free
envs inside the rounding bound of the linear integrator.  ``table(d)`` / ``report(lines)`` print the per-step figures and append
them to the file named by ``PW_TRAJECTORY_REPORT``.

Contact-free is decided on the float64 side: no colliding entity pair has come nearer than ``dist_min + 88 * contact_margin``
in that episode -- beyond that distance pw_exp's exact-zero cut makes the contact force exactly zero
(tests/test_gpu_world_constants.py::test_far_cut_where_forces_are_subnormal).  The self bit of the masks is not a contact.
"""
import os

import numpy as np

from oracle import c_oracle as co

EPS = 2.0 ** -24          # one float32 rounding, relative
EP_LEN = 25
EPISODES = 4
T_FULL = EP_LEN * EPISODES
TOL = 1e-5                # the project's per-step bar; here only a reporting threshold, never asserted on a trajectory

# The shapes of the issue: the smallest that fill more than one workgroup and leave a ragged last one.
CASES = [
    dict(id='spread3', scenario='simple_spread', num_agents=3, B=256),
    dict(id='spread6', scenario='simple_spread', num_agents=6, B=256),
    dict(id='spread9', scenario='simple_spread', num_agents=9, B=128),
    dict(id='spread12', scenario='simple_spread', num_agents=12, B=128),
    dict(id='spread24', scenario='simple_spread', num_agents=24, B=32),
    dict(id='spread48', scenario='simple_spread', num_agents=48, B=16),
    dict(id='spread4full', scenario='simple_spread', num_agents=4, B=256, obs_mode='full'),
    dict(id='tag4+2', scenario='simple_tag', num_agents=6, num_adversaries=4, B=256),
    dict(id='tag3+1', scenario='simple_tag', num_agents=4, num_adversaries=3, B=256),
    dict(id='reference', scenario='simple_reference', num_agents=2, B=256),
    dict(id='speaker_listener', scenario='simple_speaker_listener', num_agents=2, B=256),
]
# Reset seed 19: with 21 (and most others) no env of simple_spread N = 12 at B = 128 is ever contact-free -- twelve agents of
# diameter 0.3 in a 2 x 2 square nearly always start with a pair inside dist_min + 88 margins.  19 is the seed nearest to 21 that
# leaves such an env at N = 12 (one env-step) and at N = 9; every other coverage condition holds for both seeds.
SEED, ACTION_SEED = 19, 3


def is_comm(cfg):
    return cfg.scenario in (co.SIMPLE_REFERENCE, co.SIMPLE_SPEAKER_LISTENER)


def config(case, **kw):
    c = {k: v for k, v in case.items() if k not in ('id', 'B')}
    c.setdefault('max_episode_len', EP_LEN)
    c.setdefault('auto_reset', True)
    c.setdefault('seed', SEED)
    c.update(kw)
    return co.make_config(c.pop('scenario'), c.pop('num_agents'), **c)


def actions(cfg, T, B, seed=ACTION_SEED):
    """int32 index actions in the layout the env's entry takes: [T,B,N]; simple_reference [T,B,2,2] = (move, symbol);
    simple_speaker_listener [T,B,2] = (the speaker's symbol, the listener's move)."""
    rng = np.random.RandomState(seed)
    if cfg.scenario == co.SIMPLE_REFERENCE:
        return np.stack([rng.randint(0, 5, (T, B, 2)), rng.randint(0, co.DIM_C, (T, B, 2))], -1).astype(np.int32)
    if cfg.scenario == co.SIMPLE_SPEAKER_LISTENER:
        return np.stack([rng.randint(0, co.SL_DIM_C, (T, B)), rng.randint(0, 5, (T, B))], -1).astype(np.int32)
    return rng.randint(0, 5, (T, B, cfg.num_agents)).astype(np.int32)


def record(cfg, B, acts, dtype):
    """The C oracle in ``dtype`` through len(acts) steps from its reset: outputs [T, ...] and the state after every step."""
    comm = is_comm(cfg)
    o = (co.CRefOracle if comm else co.COracle)(cfg, B, dtype)
    rec = dict(obs0=o.reset(), pos0=o.pos.copy(), vel0=o.vel.copy(), lm0=o.lm.copy())
    keys = ('obs', 'final_obs', 'rew', 'rew_shared', 'done', 'terminal') + (() if comm else ('coll',))
    for k in keys + ('pos', 'vel', 'lm', 'lm_pre', 'ep_step', 'ep_count'):
        rec[k] = []
    for t in range(len(acts)):
        rec['lm_pre'].append(o.lm.copy())
        if cfg.scenario == co.SIMPLE_REFERENCE:
            w = o.step(act_idx=acts[t, :, :, 0], act_comm=acts[t, :, :, 1])
        else:
            w = o.step(act_idx=acts[t])
        if 'rew_shared' not in w:          # run.py:46: the agent-order sum, one rounding per addition in this dtype
            w['rew_shared'] = (np.zeros(B, o.dtype) + w['rew'][:, 0]) + w['rew'][:, 1]
        for k in keys:
            rec[k].append(w[k])
        for k, v in (('pos', o.pos), ('vel', o.vel), ('lm', o.lm), ('ep_step', o.ep_step), ('ep_count', o.ep_count)):
            rec[k].append(v.copy())
    for k in keys + ('pos', 'vel', 'lm', 'lm_pre', 'ep_step', 'ep_count'):
        rec[k] = np.stack(rec[k])
    if comm:
        rec['goal_final'] = o.goal.copy()
    return rec


def _eff(rec):
    """What the step produced before any reset: final_obs where the env ended its episode, obs elsewhere."""
    term = np.asarray(rec['terminal']).astype(bool)
    return np.where(term[:, :, None, None], rec['final_obs'], rec['obs'])


def _pv(cfg, obs):
    """(vel, pos) [.., N, 2] as the observation rows carry them.  simple_spread / simple_tag rows hold both verbatim
    (vel, pos, ...); the communication rows hold vel and landmark 0 - pos: there ``pos`` is that relative position."""
    return obs[..., 0:2], obs[..., 2:4]


def _sizes(cfg):
    N, L = cfg.num_agents, cfg.num_landmarks
    return np.array([cfg.agent_size[i] for i in range(N)] + [cfg.landmark_size] * L, np.float64)


class Drift(object):
    pass


_ORACLE = {}


def oracle_drift(case):
    """The float32 C oracle against the float64 one for a case of CASES over T_FULL steps: computed once, shared, read-only."""
    key = (case['id'], case['B'])
    if key not in _ORACLE:
        cfg = config(case)
        _ORACLE[key] = drift(cfg, case['B'], actions(cfg, T_FULL, case['B']))
    return _ORACLE[key]


def drift(cfg, B, acts, source=None, ref=None):
    """See the module docstring.  ``ref``: a float64 record of the same run to reuse (``oracle_drift(case).ref``)."""
    acts = np.ascontiguousarray(acts, np.int32)
    assert cfg.auto_reset and cfg.max_episode_len > 0
    ref = record(cfg, B, acts, np.float64) if ref is None else ref
    src = record(cfg, B, acts, np.float32) if source is None else source
    d = compare(cfg, B, src, ref)
    d.acts, d.from_oracle = acts, source is None
    return d


def compare(cfg, B, src, ref, start_rounded=False):
    """The differences between a float32 record and a float64 one of the same T steps (both as ``record`` lays them out; the
    float32 one may lack the per-step state).  ``start_rounded``: the float32 side started from the float64 state ROUNDED to
    float32 instead of an identical one (the B = 1 drop-in, whose reset draws float64 numbers)."""
    T, N, L = len(ref['obs']), cfg.num_agents, cfg.num_landmarks
    d = Drift()
    d.cfg, d.B, d.T, d.N, d.L, d.comm, d.ref, d.src = cfg, B, T, N, L, is_comm(cfg), ref, src
    d.from_oracle, d.start_rounded = False, start_rounded
    d.term = ref['terminal'].astype(bool)
    d.step_in_ep = np.arange(T) % cfg.max_episode_len
    e32, e64 = _eff(src).astype(np.float64), _eff(ref)
    d.e32, d.e64 = e32, e64
    d.d_obs = np.abs(e32 - e64).max(axis=(2, 3))                                   # [T,B]
    d.d_rew = np.abs(np.asarray(src['rew'], np.float64) - ref['rew']).max(axis=2)
    d.d_shared = np.abs(np.asarray(src['rew_shared'], np.float64) - ref['rew_shared'])
    v32, p32 = _pv(cfg, e32)
    v64, p64 = _pv(cfg, e64)
    d.v64, d.p64, d.v32, d.p32 = v64, p64, v32, p32
    d.dp = np.sqrt(((p32 - p64) ** 2).sum(-1))                                     # [T,B,N] Euclidean drift per agent
    d.dv = np.sqrt(((v32 - v64) ** 2).sum(-1))
    d.d_pos, d.d_vel = d.dp.max(-1), d.dv.max(-1)
    # -- float64 entity geometry per step (pre-reset), and at every episode start
    if d.comm:
        d.near = np.zeros((T, B), bool)
        d.flips = np.zeros((T, B), int)
        d.has_coll = False
    else:
        size = _sizes(cfg)
        dmin = size[:, None] + size[None, :]
        pair = np.triu(np.ones((N + L, N + L), bool), 1)
        pair[N:, :] = False                                                        # landmark-landmark: never a force
        if not cfg.landmark_collide:
            pair[:, N:] = False
        cut = dmin + 88.0 * cfg.contact_margin

        def near(pos, lm):
            ent = np.concatenate([pos, lm], axis=-2)
            dist = np.sqrt(((ent[..., :, None, :] - ent[..., None, :, :]) ** 2).sum(-1))
            return ((dist < cut) & pair).any(axis=(-1, -2)), dist
        d.near, dist = near(p64, ref['lm_pre'])
        d.dist = dist[..., :N, :N]                                                  # [T,B,N,N] agent-agent, float64
        d.dmin = dmin[:N, :N]
        # positions an episode starts from: the reset, then what each terminal step published
        start_pos = np.concatenate([ref['pos0'][None], ref['pos'][:-1]])
        start_near, _ = near(start_pos, ref['lm_pre'])
        first = d.step_in_ep == 0
        d.near = d.near | (start_near & first[:, None])
        d.has_coll = 'coll' in src
        if d.has_coll:
            x = np.asarray(src['coll']).view(np.uint64) ^ ref['coll']
            d.xor = x
            d.flips = (x != 0).any(axis=2).astype(int)
        else:
            d.flips = np.zeros((T, B), int)
    # contact so far in the episode (this step's end positions included: the stricter reading)
    d.contact = np.zeros((T, B), bool)
    run = np.zeros(B, bool)
    for t in range(T):
        if d.step_in_ep[t] == 0:
            run = np.zeros(B, bool)
        run = run | d.near[t]
        d.contact[t] = run
    return d


# ------------------------------------------------------------------------------------------------ figures
def _stats(x, sel):
    """max, 99.9th percentile, median of x over the selected envs, and the share within TOL."""
    if not sel.any():
        return (float('nan'),) * 4
    v = x[sel]
    return float(v.max()), float(np.percentile(v, 99.9)), float(np.median(v)), float((v <= TOL).mean())


def figures(d):
    """Per step t: for 'all' / 'contact' / 'free' envs the (max, p99.9, median, share <= 1e-5) of |dobs|, |drew|, |drew_shared|,
    |dpos|, |dvel|; the env counts; the number of envs whose masks differ."""
    out = []
    for t in range(d.T):
        row = dict(t=t, s=int(d.step_in_ep[t]), flips=int(d.flips[t].sum()), n_contact=int(d.contact[t].sum()),
                   n_free=int((~d.contact[t]).sum()))
        for g, sel in (('all', np.ones(d.B, bool)), ('contact', d.contact[t]), ('free', ~d.contact[t])):
            for name, x in (('obs', d.d_obs), ('rew', d.d_rew), ('shared', d.d_shared), ('pos', d.d_pos), ('vel', d.d_vel)):
                row[g + '_' + name] = _stats(x[t], sel)
        out.append(row)
    return out


def horizon(d):
    """(first step index within an episode at which any env exceeds 1e-5 in any episode, or None;
    the smallest share of envs within 1e-5 at the last step of an episode; the worst |dobs| of the run)."""
    over = (d.d_obs > TOL).any(axis=1)
    steps = sorted(set(d.step_in_ep[over].tolist()))
    last = d.step_in_ep == d.cfg.max_episode_len - 1
    return (steps[0] if steps else None), float((d.d_obs[last] <= TOL).mean(axis=1).min()), float(d.d_obs.max())


def table(d, title, episode=EPISODES - 1):
    """The per-step figures of one episode (the fourth by default) and the run's horizon, as text lines."""
    fig = figures(d)
    first, share, worst = horizon(d)
    pos = '|d(lm0-pos)|' if d.comm else '|dpos|'
    lines = ['# %s  B=%d N=%d L=%d T=%d  flips(all steps)=%d  first step index over 1e-5: %s  share<=1e-5 at step %d: %.1f %%  '
             'worst |dobs| %.2e' % (title, d.B, d.N, d.L, d.T, int(d.flips.sum()), 'none' if first is None else first,
                                    d.cfg.max_episode_len - 1, 100 * share, worst),
             '#  episode %d; columns: step | all envs: max p99.9 median share<=1e-5 of |dobs| | contact envs: count max|dobs| | '
             'contact-free envs: count max|dobs| | max|drew| max|drew_shared| | envs with mask flips | max%s max|dvel|' % (episode + 1, pos)]
    for r in fig[episode * d.cfg.max_episode_len:(episode + 1) * d.cfg.max_episode_len]:
        a = r['all_obs']
        lines.append('%3d | %.2e %.2e %.2e %6.1f%% | %4d %.2e | %4d %.2e | %.2e %.2e | %3d | %.2e %.2e' % (
            r['s'], a[0], a[1], a[2], 100 * a[3], r['n_contact'], r['contact_obs'][0], r['n_free'], r['free_obs'][0],
            r['all_rew'][0], r['all_shared'][0], r['flips'], r['all_pos'][0], r['all_vel'][0]))
    return lines


def report(lines):
    path = os.environ.get('PW_TRAJECTORY_REPORT')
    for l in lines:
        print(l)
    if path:
        with open(path, 'a') as f:
            f.write('\n'.join(lines) + '\n')


# ------------------------------------------------------------------------------------------------ structural assertions
def _half_ulp32(x64):
    """One float32 rounding of a float64 value: half the spacing of float32 at it."""
    return 0.5 * np.spacing(np.abs(x64).astype(np.float32)).astype(np.float64)


def check_reset(d):
    """After every reset (the first and each auto-reset) the float32 state cast to float64 equals the float64 state exactly;
    the observation rows differ by at most one float32 rounding of each component (the state is float32-representable in both:
    the differences lm - pos are exact in float64 and rounded once in float32)."""
    src, ref = d.src, d.ref
    resets = [(-1, src['obs0'], ref['obs0'])] + [(t, src['obs'][t], ref['obs'][t]) for t in range(d.T) if d.term[t].any()]
    assert len(resets) == 1 + d.T // d.cfg.max_episode_len
    for t, o32, o64 in resets:
        if t >= 0:
            assert d.term[t].all()
        o32 = np.asarray(o32, np.float64)
        bad = np.abs(o32 - o64) > _half_ulp32(o64)
        assert not bad.any(), 'reset after step %d: %d observation entries differ by more than one float32 rounding' % (t, bad.sum())
        assert np.array_equal(o32[..., 0:2], o64[..., 0:2]) and not o64[..., 0:2].any(), 'reset after step %d: velocities' % t
        if not d.comm:
            assert np.array_equal(o32[..., 2:4], o64[..., 2:4]), 'reset after step %d: positions' % t
    states = []
    if d.from_oracle:
        states.append((src['pos0'], src['vel0'], src['lm0'], ref['pos0'], ref['vel0'], ref['lm0']))
        states += [(src['pos'][t], src['vel'][t], src['lm'][t], ref['pos'][t], ref['vel'][t], ref['lm'][t])
                   for t in range(d.T) if d.term[t].any()]
    elif 'final_state' in src and d.term[d.T - 1].all():
        st = src['final_state']
        states.append((st['pos'], st['vel'], st['landmarks'], ref['pos'][-1], ref['vel'][-1], ref['lm'][-1]))
    for s in states:
        for a, b in zip(s[:3], s[3:]):
            assert np.array_equal(np.asarray(a, np.float64), b), 'reset state differs between float32 and float64'
    return len(resets), len(states)


def check_clocks(d):
    src, ref = d.src, d.ref
    assert np.array_equal(np.asarray(src['terminal']).astype(np.uint8), ref['terminal']), 'terminal'
    assert np.array_equal(np.asarray(src['done']).astype(np.uint8), ref['done']) and not ref['done'].any(), 'done'
    want = (d.step_in_ep == d.cfg.max_episode_len - 1)
    assert np.array_equal(d.term, np.repeat(want[:, None], d.B, 1))
    if 'ep_step' in src:
        assert np.array_equal(np.asarray(src['ep_step']), ref['ep_step']), 'ep_step'
        assert np.array_equal(np.asarray(src['ep_count']).astype(np.uint32), ref['ep_count']), 'ep_count'
    if 'final_state' in src:
        st = src['final_state']
        assert np.array_equal(np.asarray(st['ep_step']), ref['ep_step'][-1]), 'ep_step (final state)'
        assert np.array_equal(np.asarray(st['ep_count']).astype(np.uint32), ref['ep_count'][-1]), 'ep_count (final state)'


def check_mask_flips(d):
    """A collision-mask bit may differ from float64 only for a pair whose float64 distance is closer to dist_min than the two
    agents' combined position drift at that step (|d32 - d64| <= |dp_i| + |dp_j|: triangle inequality) plus one float32 ulp of the
    distance.  -> number of flipped (step, env, pair) bits."""
    if d.comm or not d.has_coll:
        return 0
    N = d.N
    bits = ((d.xor[..., None] >> np.arange(N, dtype=np.uint64)) & np.uint64(1)).astype(bool)     # [T,B,i,j]
    t, b, i, j = np.nonzero(bits)
    gap = np.abs(d.dist[t, b, i, j] - d.dmin[i, j])
    band = d.dp[t, b, i] + d.dp[t, b, j] + np.spacing(d.dist[t, b, i, j].astype(np.float32)).astype(np.float64)
    bad = gap > band
    assert not bad.any(), 'mask bits flipped outside the drift band: %s' % (
        [(int(t[k]), int(b[k]), int(i[k]), int(j[k]), float(gap[k]), float(band[k])) for k in np.nonzero(bad)[0][:5]],)
    assert (i != j).all(), 'a self bit flipped'
    return len(t)


def reward_bound(d):
    """[T,B,N]: Lipschitz constant of the scenario's reward in the agent positions x that step's measured position drift, plus the
    float32 rounding of the sum, (term count) x 2^-24 x sum |terms|.  Valid in envs whose masks agree with float64.

    simple_spread   rew_i = - sum_l min_a |p_a - lm_l| - #(mask bits of i).  Landmarks are identical in both precisions (reset
        check) and |min_a f_a - min_a g_a| <= max_a |f_a - g_a|, | |p - lm| - |p' - lm| | <= |p - p'|: every one of the L terms moves
        by at most D = max_a |dp_a|, the integer term not at all.  Lipschitz constant L in D.  Terms: L distances and the set bits.
    simple_tag      adversary: 10 x #(colliding good-adversary pairs): the bits of the masks, exact -> bound 0.
        good agent: -10 x #(adversary bits) - bound(|x|) - bound(|y|); bound() is continuous, slope 10 on [0.9, 1) and
        2 exp(2x - 2) <= 20 beyond, where min(., 10) caps it (the cap is reached at exp(.) = 10: slope 20): 20 (|dx| + |dy|) <=
        20 sqrt(2) |dp_i|.  Terms: the bits (10 each) and, per coordinate past 0.9 - drift, the operands of the penalty:
        (x - 0.9) 10 has 10 |x| and 9 (0.9 itself is rounded to float32), exp(2x - 2) <= 10 has relative error (2|x| + 2) roundings
        of its argument plus pw_exp's own 1.5 ulp (profiles/r2_math_accuracy.txt): max(10, 2 b) (|x| + 1) covers both.
    simple_reference / simple_speaker_listener   rew = -|q|^2, q = p_other - lm_goal (both observed: q is minus a landmark column of
        the other agent's row).  |q|^2 - |q'|^2 = (q - q') . (q + q') <= |dq| (2 |q| + |dq|).  Terms: q_x^2, q_y^2, each with the
        rounding of q (a difference: operands |p|, |lm|, bounded by |q| + 2 |lm| <= |q| + 2), of the square and of the sum.
    """
    cfg, T, B, N, L = d.cfg, d.T, d.B, d.N, d.L
    r64 = d.ref['rew']
    if cfg.scenario == co.SIMPLE_SPREAD:
        D = d.dp.max(-1)[:, :, None]
        nbits = np.array([[[bin(int(m)).count('1') for m in row] for row in step] for step in d.ref['coll']], np.float64)
        terms = L + nbits
        # a rounded start (compare(start_rounded=True)) also rounds each landmark once: sqrt(2) 2^-24 |lm| per distance term
        lm_round = L * np.sqrt(2.0) * EPS * np.abs(d.ref['lm_pre']).max() if d.start_rounded else 0.0
        return L * D + lm_round + terms * EPS * np.abs(r64)  # every term has the reward's sign: sum |terms| = |rew|
    if cfg.scenario == co.SIMPLE_TAG:
        A = cfg.num_adversaries
        x = np.abs(d.p64)                                   # [T,B,N,2]
        b = np.where(x < 0.9, 0.0, np.where(x < 1.0, (x - 0.9) * 10, np.minimum(np.exp(2 * x - 2), 10.0)))
        close = x >= 0.9 - d.dp[..., None]
        opnd = np.where(close, np.maximum(10.0, 2 * b) * (x + 1.0), 0.0).sum(-1)
        nbits = np.array([[[bin(int(m) & ((1 << A) - 1)).count('1') for m in row] for row in step] for step in d.ref['coll']], np.float64)
        terms = nbits + 6 * close.sum(-1)              # per coordinate: |x|, the argument, exp (1.5 ulp = 3 x 2^-24) or constant + product, the sum
        bound = 20.0 * np.sqrt(2.0) * d.dp + terms * EPS * (10.0 * nbits + opnd)
        bound[:, :, :A] = 0.0
        return bound
    # communication scenarios: the observed q of the agent whose position the reward reads
    sl = cfg.scenario == co.SIMPLE_SPEAKER_LISTENER
    goal = _goals(d)                                        # [T,B,N] landmark index each agent's reward reads
    other = np.array([1, 1] if sl else [1, 0])
    lmcols = d.e64[..., 2:2 + 2 * L].reshape(T, B, N, L, 2)
    lm32 = d.e32[..., 2:2 + 2 * L].reshape(T, B, N, L, 2)
    tt, bb = np.meshgrid(np.arange(T), np.arange(B), indexing='ij')
    bound = np.zeros((T, B, N))
    for i in range(N):
        q64 = lmcols[tt, bb, other[i], goal[:, :, i]]       # [T,B,2]
        q32 = lm32[tt, bb, other[i], goal[:, :, i]]
        dq = np.sqrt(((q32 - q64) ** 2).sum(-1))
        qn = np.sqrt((q64 ** 2).sum(-1))
        bound[:, :, i] = dq * (2 * qn + dq) + 2 * 3 * EPS * (qn + 2.0) ** 2
    return bound


def _goals(d):
    """The landmark each agent's reward reads, per step, recovered on the float64 side from the reward itself: the landmark l
    for which -|q_l|^2 equals the float64 reward (exact match to 1e-12; goals change only at resets)."""
    cfg, T, B, N, L = d.cfg, d.T, d.B, d.N, d.L
    sl = cfg.scenario == co.SIMPLE_SPEAKER_LISTENER
    other = [1, 1] if sl else [1, 0]
    lmcols = d.e64[..., 2:2 + 2 * L].reshape(T, B, N, L, 2)
    goal = np.zeros((T, B, N), int)
    for i in range(N):
        cand = -(lmcols[:, :, other[i]] ** 2).sum(-1)       # [T,B,L]
        err = np.abs(cand - d.ref['rew'][:, :, i, None])
        goal[:, :, i] = err.argmin(-1)
        assert (err.min(-1) <= 1e-12).all()
    return goal


def check_rewards(d):
    """|drew| within reward_bound in every env whose masks agree with float64 (a flipped bit is a step of 1 or 10, not rounding).
    -> the largest |drew| / bound seen (reported, not asserted beyond <= 1)."""
    ok = np.repeat((d.flips == 0)[:, :, None], d.N, 2)
    bound = reward_bound(d)
    err = np.abs(np.asarray(d.src['rew'], np.float64) - d.ref['rew'])
    bad = ok & (err > bound)
    assert not bad.any(), 'rewards outside the Lipschitz bound: %s' % (
        [(int(t), int(b), int(i), float(err[t, b, i]), float(bound[t, b, i])) for t, b, i in zip(*np.nonzero(bad))][:5],)
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(ok & (bound > 0), err / bound, 0.0)
    return float(ratio.max())


def free_bound(d):
    """Worst-case rounding bound of the contact-free integrator, per step, env (its own running max |p|, max |v|) and agent, in
    the Euclidean norm: (ev, ep) [T,B].

    Without a contact force an agent obeys v' = (1 - damping) v + a dt / m, p' = p + v' dt with |a| = its sensitivity (or 0).
    Float32 against exact arithmetic, per component, e = 2^-24:
        v (1 - damping)      one rounding of the product (+ one of 1 - damping):      2 e |v|
        a dt / m             sensitivity x action, / m, x dt, dt's own rounding:      4 e |a| dt / m
        the sum v'           one rounding:                                             e |v'|
        p + v' dt            product, dt's rounding, sum:                              2 e |v'| dt + e |p'|
    and the inherited error contracts by (1 - damping) in v and carries over unchanged in p.  simple_tag's speed clamp is the
    projection onto a disc -- non-expansive in the Euclidean norm -- computed with a sqrt of a two-term sum, a division and a
    product: 5 e max_speed more.  Components -> Euclidean norm: sqrt(2).  The communication rows carry lm_0 - pos instead of
    pos: one more rounding of that difference, and |pos| <= |lm_0 - pos| + 1."""
    cfg, T, B, N = d.cfg, d.T, d.B, d.N
    damp, dt, mass = 1.0 - cfg.damping, cfg.dt, cfg.mass
    a = np.array([cfg.agent_accel[i] if cfg.agent_accel[i] >= 0 else cfg.default_sensitivity for i in range(N)]).max() / mass
    ms = max([cfg.agent_max_speed[i] for i in range(N)] + [0.0])
    r2 = np.sqrt(2.0)
    ev, ep = np.zeros((T, B)), np.zeros((T, B))
    cur_v, cur_p = np.zeros(B), np.zeros(B)
    vmax, pmax = np.zeros(B), np.zeros(B)
    for t in range(T):
        if d.step_in_ep[t] == 0:
            vmax = np.zeros(B)
            start = d.ref['obs0'] if t == 0 else d.ref['obs'][t - 1]          # what the episode starts from
            pmax = np.abs(start[..., 2:4]).reshape(B, -1).max(-1)
            cur_v, cur_p = np.zeros(B), (r2 * EPS * pmax if d.start_rounded else np.zeros(B))
        vmax = np.maximum(vmax, np.maximum(np.abs(d.v64[t]), np.abs(d.v32[t])).reshape(B, -1).max(-1))
        pmax = np.maximum(pmax, np.maximum(np.abs(d.p64[t]), np.abs(d.p32[t])).reshape(B, -1).max(-1))
        pm = pmax + 1.0 if d.comm else pmax
        cur_v = damp * cur_v + r2 * EPS * (2 * vmax + 4 * a * dt + vmax + 5 * ms)
        cur_p = cur_p + dt * cur_v + r2 * EPS * (2 * vmax * dt + pm)
        ev[t], ep[t] = cur_v, cur_p + (r2 * EPS * pmax if d.comm else 0.0)
    return ev, ep


def check_contact_free(d):
    """Every agent of a contact-free env stays inside free_bound.  -> (largest |dv| / bound, largest |dp| / bound) over them."""
    ev, ep = free_bound(d)
    free = ~d.contact
    bad_v = free[:, :, None] & (d.dv > ev[:, :, None])
    bad_p = free[:, :, None] & (d.dp > ep[:, :, None])
    for name, bad, x, bnd in (('velocity', bad_v, d.dv, ev), ('position', bad_p, d.dp, ep)):
        assert not bad.any(), 'contact-free env drifts like a contact one (%s): %s' % (
            name, [(int(t), int(b), int(i), float(x[t, b, i]), float(bnd[t, b])) for t, b, i in zip(*np.nonzero(bad))][:5])
    if not free.any():
        return 0.0, 0.0
    return float((d.dv.max(-1) / ev)[free].max()), float((d.dp.max(-1) / ep)[free].max())


def check_structure(d):
    """Every structural assertion; -> dict of the counts and slack ratios for the report."""
    resets, states = check_reset(d)
    check_clocks(d)
    flipped = check_mask_flips(d)
    rr = check_rewards(d)
    rv, rp = check_contact_free(d)
    return dict(resets=resets, reset_states=states, flipped_bits=flipped, reward_ratio=rr, free_vel_ratio=rv, free_pos_ratio=rp,
                envs_with_flips=int(d.flips.sum()), free_env_steps=int((~d.contact).sum()), contact_env_steps=int(d.contact.sum()))


def summary_line(title, info):
    return ('# %s structure: %d resets (%d states compared exactly), %d mask bits flipped inside the drift band (%d env-steps), '
            'worst |drew| / bound %.3f, contact-free worst |dv| / bound %.3f, |dp| / bound %.3f, %d contact-free and %d contact env-steps'
            % (title, info['resets'], info['reset_states'], info['flipped_bits'], info['envs_with_flips'], info['reward_ratio'],
               info['free_vel_ratio'], info['free_pos_ratio'], info['free_env_steps'], info['contact_env_steps']))
