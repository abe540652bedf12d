"""pw_spread_quad_kernel with the collision half of the reward wave's step moved to wave OB (counts handed over through two LDS words per
lane, one step later; the launch's last count computed by wave OA itself; the collision masks stored by OB): every output plane, `coll`
where requested, and the carried state equal the one-wave stream kernel's bit for bit, over every env and every step, at the smallest
shapes at which the hand-over can go wrong."""
import pytest

torch = pytest.importorskip('torch')

AUTO = dict(force_generic=0, no_stream=0, duo=-1, quad=-1, obs_block=-1, trio=-1, p_prio=-1, envs_per_wave=0, policy_form=0)
N = 6
OUTS = ('obs', 'rew', 'rew_shared', 'done', 'terminal')
STATE = ('pos', 'vel', 'landmarks', 'ep_step', 'ep_count')


def _same(a, b, name):
    """Bitwise by the suite's rule (tests/test_gpu_quad_stream.py _same): float tensors as their int32 patterns, a NaN equals a NaN."""
    assert a.shape == b.shape and a.dtype == b.dtype, (name, a.shape, b.shape, a.dtype, b.dtype)
    if a.dtype.is_floating_point:
        same = (a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)) | (torch.isnan(a) & torch.isnan(b))
        assert bool(same.all()), (name, int((~same).sum()))
    else:
        assert torch.equal(a, b), name


def _both(B, launches, ep_len=25, want_coll=False, edit_state=None, desync=True, idle_actions=False):
    """The same start state and actions through the stream kernel and the quad kernel, `launches` (a tuple of step counts) consecutive
    rollouts into one handle each (in the manner of tests/test_gpu_quad_stream.py _both).  -> {form: ([outputs per launch], state after)}"""
    from multiagent_rl_amd.env import BatchedParticleEnv
    gen = torch.Generator().manual_seed(1000 * B + sum(launches))
    acts = [torch.randint(0, 5, (T, B, N), dtype=torch.int32, generator=gen).cuda() for T in launches]
    if idle_actions:
        acts = [torch.zeros_like(a) for a in acts]
    res = {}
    for form, disp, kernel in (('stream', dict(AUTO, duo=0), 'pw_spread_stream_kernel'), ('quad', dict(AUTO, quad=1), 'pw_spread_quad_kernel')):
        env = BatchedParticleEnv('simple_spread', B, num_agents=N, max_episode_len=ep_len, auto_reset=True, seed=41, want_coll=want_coll,
                                 dispatch=disp)
        env.reset()
        st = env.get_state()
        pos, vel = st['pos'] * 0.3, st['vel']   # crowded: contacts in most steps
        if edit_state is not None:
            pos, vel = edit_state(pos.clone(), vel.clone())
        ep_step = ((torch.arange(B, device='cuda') * 7) % ep_len).int() if desync else st['ep_step']
        env.set_state(pos, vel, st['landmarks'], ep_step=ep_step, ep_count=st['ep_count'])
        outs = []
        for a in acts:
            o = env.rollout(a)
            outs.append({k: v.clone() for k, v in o.items()})
            assert env.last_kernel().startswith(kernel), env.last_kernel()
        res[form] = (outs, env.get_state())
    return res


def _check(res, want_coll=False):
    (sa, sta), (qa, stq) = res['stream'], res['quad']
    for i, (a, b) in enumerate(zip(sa, qa)):
        for k in OUTS:
            _same(a[k], b[k], '%s of launch %d' % (k, i))
        term = a['terminal'].bool()
        if term.any():
            _same(a['final_obs'][term], b['final_obs'][term], 'final_obs of launch %d' % i)
        if want_coll:
            _same(a['coll'], b['coll'], 'coll of launch %d' % i)
    for k in STATE:
        _same(sta[k], stq[k], 'state %s' % k)
    return sa


@pytest.mark.gpu
@pytest.mark.parametrize('B', [1, 7, 9, 13])
@pytest.mark.parametrize('launches', [(1,), (2,), (3,), (1, 1, 2), (5, 4)], ids=lambda s: '+'.join(map(str, s)))
def test_counts_handed_over_at_both_parities_and_the_peeled_last_step(B, launches):
    """T = 1: the launch is wave OA's epilogue alone (its own count, nothing read from LDS); 2 and 3: the first hand-over through each of
    the two buffers, then the peeled last step; (1, 1, 2) and (5, 4): state carried across launches that end on different parities.
    B = 1 / 7: one partial workgroup (the second physics wave idle / with three envs); 9 / 13: a full workgroup and a partial one."""
    _check(_both(B, launches, ep_len=25))


@pytest.mark.gpu
@pytest.mark.parametrize('want_coll', [False, True], ids=['plain', 'coll'])
@pytest.mark.parametrize('ep_len', [2, 3])
def test_a_terminal_steps_count_comes_from_the_pre_reset_slot(ep_len, want_coll):
    """Desynchronised clocks, episodes of 2 and 3 steps: resets fall in consecutive steps, every such step publishes two ring slots, and
    the count (and the mask) of a terminal step belongs to the state BEFORE the reset.  Odd and even step counts, two launches."""
    outs = _check(_both(13, (7, 4), ep_len=ep_len, want_coll=want_coll), want_coll=want_coll)
    term = outs[0]['terminal'].bool()
    assert term.any() and not term.all()


FAR = [(3.0, 3.0), (-3.0, 3.0), (3.0, -3.0), (-3.0, -3.0), (0.0, 4.5), (0.0, -4.5)]   # pairwise 3 apart and more: nobody collides here


def _clusters(pos, vel):
    """Every agent far from every other, at rest -- but a pair in env 1 and a triple in env 4 that approach each other at unit speed
    and, with idle actions, overlap in the second step (damping 0.25, dt 0.1: the pair's 0.5 of separation shrinks to 0.35, then to
    0.2375; the triple's circle of radius 0.29 to one of 0.159, pairwise 0.275; the collision distance is 0.3).  Env 6: a NaN."""
    far = torch.tensor(FAR, device=pos.device)
    pos[:] = far
    vel[:] = 0.0
    pos[1, 0] = torch.tensor([-0.25, 0.0]); vel[1, 0] = torch.tensor([1.0, 0.0])
    pos[1, 1] = torch.tensor([0.25, 0.0]); vel[1, 1] = torch.tensor([-1.0, 0.0])
    for i, (cx, cy) in enumerate([(1.0, 0.0), (-0.5, 0.8660254), (-0.5, -0.8660254)]):
        pos[4, i] = torch.tensor([0.29 * cx, 0.29 * cy])
        vel[4, i] = torch.tensor([-cx, -cy])
    pos[6, 3, 0] = float('nan')
    return pos, vel


@pytest.mark.gpu
def test_real_collisions_counts_of_one_two_and_three():
    """The stream kernel's own rewards show the counts: within an env every agent's reward is minus the same sum of landmark distances
    minus its count, and each env here keeps an isolated agent (count 1, itself), so count = 1 + (the env's largest reward - its own).
    The env with a NaN coordinate: the agent fails its own test -- bit `agent` of its mask is clear, in both kernels."""
    res = _both(9, (4,), ep_len=25, want_coll=True, edit_state=_clusters, desync=False, idle_actions=True)
    outs = _check(res, want_coll=True)
    rew = outs[0]['rew']                                  # [T, B, N], the stream kernel's
    fin = torch.isfinite(rew).all(dim=2)                  # envs without the NaN
    counts = 1 + torch.round(rew.max(dim=2, keepdim=True).values - rew)
    seen = set(counts[fin].flatten().tolist())
    print('collision counts the stream kernel reports:', sorted(seen))
    assert {1.0, 2.0, 3.0} <= seen, seen
    coll = outs[0]['coll']
    assert int(coll[1, 1, 0]) & 0x3f == 0b000011 and int(coll[1, 4, 2]) & 0x3f == 0b000111, (coll[1, 1], coll[1, 4])
    assert int(coll[0, 6, 3]) & (1 << 3) == 0 and int(coll[0, 0, 3]) & 0x3f == 1 << 3, (coll[0, 6], coll[0, 0])
