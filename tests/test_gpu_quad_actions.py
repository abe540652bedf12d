"""pw_spread_quad_kernel's action force: wave OB fetches the action indices, looks the force up and hands it to the physics waves through
a two-slot ring in LDS, two steps ahead; the physics waves supply steps 0 and 1 of a launch themselves.  Every output of every launch and
the state after it equal the one-wave stream kernel's bit for bit (in the manner of tests/test_gpu_quad_balance.py), at the smallest shapes
at which the hand-over can go wrong: launches that end before OB has supplied anything, both slot parities, a physics wave that idles,
a partial workgroup, reset steps in consecutive iterations, indices outside 0..4, and a world whose force table is not the canonical one.
Nothing here depends on which wave does the work: the file passes on the kernel as it was before the move as well."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

from tests import world_constants as wc  # noqa: E402

AUTO = dict(force_generic=0, no_stream=0, duo=-1, quad=-1, obs_block=-1, trio=-1, p_prio=-1, envs_per_wave=0, policy_form=0)
N = 6
OUTS = ('obs', 'rew', 'rew_shared', 'done', 'terminal')
STATE = ('pos', 'vel', 'landmarks', 'ep_step', 'ep_count')
FORMS = (('stream', dict(AUTO, duo=0), 'pw_spread_stream_kernel'), ('quad', dict(AUTO, quad=1), 'pw_spread_quad_kernel'))
LAUNCHES = [(1,), (2,), (3,), (1, 1, 2), (4, 5), (9,)]
SEQ_IDS = lambda s: '+'.join(map(str, s))  # noqa: E731


def _same(a, b, name):
    """Bitwise by the suite's rule (tests/test_gpu_quad_stream.py _same): float tensors as their int32 patterns, a NaN equals a NaN."""
    assert a.shape == b.shape and a.dtype == b.dtype, (name, a.shape, b.shape, a.dtype, b.dtype)
    if a.dtype.is_floating_point:
        same = (a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)) | (torch.isnan(a) & torch.isnan(b))
        assert bool(same.all()), (name, int((~same).sum()))
    else:
        assert torch.equal(a, b), name


def _uniform(B, launches):
    gen = torch.Generator().manual_seed(7000 * B + 13 * sum(launches) + len(launches))
    return [torch.randint(0, 5, (T, B, N), dtype=torch.int32, generator=gen) for T in launches]


def _ramp(B, launches):
    """Every agent's index at step t (counted over the launches) is t mod 5: a slot or step off by one changes every force."""
    t0, acts = 0, []
    for T in launches:
        acts.append(((torch.arange(t0, t0 + T, dtype=torch.int32) % 5)[:, None, None]).expand(T, B, N).contiguous())
        t0 += T
    return acts


def _both(B, acts, ep_len=25, want_coll=False, world=None, constants=None):
    """The same start state and actions through the stream kernel and the quad kernel, one rollout per tensor of `acts` into one
    handle each.  `world`: a constant set of tests/world_constants.py; `constants`: world constants by name.
    -> {form: ([outputs per launch], state after, kernel name)}"""
    from multiagent_rl_amd.env import BatchedParticleEnv
    res = {}
    for form, disp, kernel in FORMS:
        run = dict(max_episode_len=ep_len, auto_reset=True, seed=43)
        if world is not None:
            pw, _ = wc.both_configs(world, 'simple_spread', B, N, **run)
            env = BatchedParticleEnv('simple_spread', config=pw, want_coll=want_coll, dispatch=disp)
        else:
            env = BatchedParticleEnv('simple_spread', B, num_agents=N, want_coll=want_coll, dispatch=disp, **dict(run, **(constants or {})))
        env.reset()
        st = env.get_state()
        ep_step = ((torch.arange(B, device='cuda') * 7) % ep_len).int()   # desynchronised clocks
        env.set_state(st['pos'] * 0.3, st['vel'], st['landmarks'], ep_step=ep_step, ep_count=st['ep_count'])   # crowded: contacts in most steps
        outs = []
        for a in acts:
            o = env.rollout(a.cuda())
            outs.append({k: v.clone() for k, v in o.items()})
            assert env.last_kernel().startswith(kernel), env.last_kernel()
        res[form] = (outs, env.get_state(), env.last_kernel())
    return res


def _check(res, want_coll=False):
    (sa, sta, _), (qa, stq, _) = res['stream'], res['quad']
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


@pytest.mark.parametrize('B', [4, 8, 13, 20])
@pytest.mark.parametrize('launches', LAUNCHES, ids=SEQ_IDS)
def test_every_launch_sequence_at_every_batch_shape(B, launches):
    """(1,), (2,): the launch ends before wave OB has supplied a force; (3,): the first hand-over; (1, 1, 2) and (4, 5): state carried
    over launches that end on either slot parity; (9,): the steady state.  B = 4: the second physics wave idles; 8: one full
    workgroup; 13: a partial last workgroup whose second physics wave has one env; 20: two full workgroups and half of one.
    Episodes of 25 steps with desynchronised clocks (some env resets in most launches).  Seeded uniform indices, then the ramp."""
    _check(_both(B, _uniform(B, launches)))
    _check(_both(B, _ramp(B, launches)))


@pytest.mark.parametrize('want_coll', [False, True], ids=['plain', 'coll'])
@pytest.mark.parametrize('ep_len', [2, 3])
def test_reset_steps_in_consecutive_iterations(ep_len, want_coll):
    """Episodes of 2 and 3 steps, desynchronised: resets in consecutive steps, every such step publishes two ring slots of the state --
    and still consumes ONE action force.  Both instantiations of the collision-mask switch; the ramp plane, odd and even launches."""
    outs = _check(_both(13, _ramp(13, (4, 5)), ep_len=ep_len, want_coll=want_coll), want_coll=want_coll)
    term = outs[1]['terminal'].bool()
    assert term.any() and not term.all()
    _check(_both(20, _uniform(20, (9,)), ep_len=ep_len, want_coll=want_coll), want_coll=want_coll)


def test_indices_outside_the_five_actions_give_no_force():
    """The Python layer passes int32 indices through unchecked, so 5, 9 and -1 reach the kernels: every kernel treats them as `no
    force` (the quad kernel through entry 5 of its table, behind an unsigned clamp).  A few lanes, in the physics waves' own steps
    (0 and 1) and in wave OB's."""
    B, launches = 13, (4, 5)
    acts = _uniform(B, launches)
    for a in acts:
        for t in range(a.shape[0]):
            a[t, (3 * t) % B, t % N] = 5
            a[t, (3 * t + 1) % B, (t + 2) % N] = 9
            a[t, (3 * t + 7) % B, (t + 4) % N] = -1
    outs = _check(_both(B, acts))
    # the force really is none: the same launches with index 0 (no-op) in those lanes give the same bits
    noop = [torch.where((a < 0) | (a > 4), torch.zeros_like(a), a) for a in acts]
    ref = _both(B, noop)['stream'][0]
    for i, (a, b) in enumerate(zip(outs, ref)):
        _same(a['obs'], b['obs'], 'obs of launch %d against the no-op plane' % i)


def test_the_unit_world_builds_another_force_table():
    """tests/world_constants.py `unit`: unit mass (the quad kernel needs it) with action_force_uses_accel and an acceleration of 2.5,
    i.e. a force scale and table entries of their own, built with the step's expressions."""
    for B in (8, 13):
        res = _both(B, _ramp(B, (4, 5)), ep_len=3, want_coll=True, world='unit')
        _check(res, want_coll=True)
        canon = _both(B, _ramp(B, (4, 5)), ep_len=3, want_coll=True)
        assert not torch.equal(res['quad'][0][0]['obs'], canon['quad'][0][0]['obs'])   # the constants did reach the kernel


def test_a_margin_that_needs_the_full_division():
    """A contact margin whose significand is all ones: the host's margin test (pw_margin_one_correction) fails, K1 is false."""
    from multiagent_rl_amd import _lib
    margin = float(np.float32(0.0009765624417923391))
    assert _lib.load().pw_margin_one_correction(C.c_float(margin)) == 0
    for want_coll in (False, True):
        res = _both(13, _uniform(13, (4, 5)), ep_len=3, want_coll=want_coll, constants=dict(contact_margin=margin))
        _check(res, want_coll=want_coll)
