"""pw_spread_quad_kernel's reset draws ahead: wave OB draws the next episode's agent and landmark positions in slices during the episode
and leaves them in LDS; a reset step in which every env of the workgroup restarts, at least QUAD_DRAW_DEPTH steps after the pipeline's
start, takes them from there (csrc/pw_kernels_spread_quad.hpp, "Reset draws ahead").  Every output of every launch and the state after it
equal the one-wave stream kernel's bit for bit (in the manner of tests/test_gpu_quad_actions.py).  The other quad tests desynchronise the
episode clocks and so never reach that path; here the clocks are equal, per workgroup at least, and the cases sit where the path is taken,
just not taken, and left again: resets just before, at and behind the depth, episodes shorter than the pipeline, clocks apart by one step
in one env, clocks made equal between two launches, episode counts and env ids of every lane's own.
Nothing here depends on where the draws are made: the file passes on the kernel as it was before the change as well."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

from multiagent_rl_amd.env import QUAD_DRAW_DEPTH as D  # noqa: E402
from tests import world_constants as wc  # noqa: E402

AUTO = dict(force_generic=0, no_stream=0, duo=-1, quad=-1, obs_block=-1, trio=-1, p_prio=-1, envs_per_wave=0, policy_form=0)
N = 6
OUTS = ('obs', 'rew', 'rew_shared', 'done', 'terminal')
STATE = ('pos', 'vel', 'landmarks', 'ep_step', 'ep_count')
FORMS = (('stream', dict(AUTO, duo=0), 'pw_spread_stream_kernel'), ('quad', dict(AUTO, quad=1), 'pw_spread_quad_kernel'))
SEQ_IDS = lambda s: '+'.join(map(str, s))  # noqa: E731
EP = 12


def _same(a, b, name):
    """Bitwise by the suite's rule (tests/test_gpu_quad_stream.py _same): float tensors as their int32 patterns, a NaN equals a NaN."""
    assert a.shape == b.shape and a.dtype == b.dtype, (name, a.shape, b.shape, a.dtype, b.dtype)
    if a.dtype.is_floating_point:
        same = (a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)) | (torch.isnan(a) & torch.isnan(b))
        assert bool(same.all()), (name, int((~same).sum()))
    else:
        assert torch.equal(a, b), name


def _uniform(B, launches):
    gen = torch.Generator().manual_seed(9000 * B + 13 * sum(launches) + len(launches))
    return [torch.randint(0, 5, (T, B, N), dtype=torch.int32, generator=gen) for T in launches]


def _ramp(B, launches):
    """Every agent's index at step t (counted over the launches) is t mod 5."""
    t0, acts = 0, []
    for T in launches:
        acts.append(((torch.arange(t0, t0 + T, dtype=torch.int32) % 5)[:, None, None]).expand(T, B, N).contiguous())
        t0 += T
    return acts


def _both(B, acts, ep_len=EP, clocks=0, reclock=None, ep_count=None, want_coll=False, world=None, constants=None, **run_kw):
    """The same start state and actions through the stream kernel and the quad kernel, one rollout per tensor of `acts` into one handle
    each.  `clocks`: the episode clocks at the start (a number: the same for every env); `reclock`: {launch index: clocks} set, with the
    rest of the state kept, before that launch; `ep_count`: episode counts at the start.
    -> {form: ([outputs per launch], state after, kernel name)}"""
    from multiagent_rl_amd.env import BatchedParticleEnv
    res = {}
    as_clocks = lambda c: (torch.full((B,), c) if isinstance(c, int) else torch.as_tensor(c)).int().cuda()  # noqa: E731
    for form, disp, kernel in FORMS:
        run = dict(max_episode_len=ep_len, auto_reset=True, seed=43, **run_kw)
        if world is not None:
            pw, _ = wc.both_configs(world, 'simple_spread', B, N, **run)
            env = BatchedParticleEnv('simple_spread', config=pw, want_coll=want_coll, dispatch=disp)
        else:
            env = BatchedParticleEnv('simple_spread', B, num_agents=N, want_coll=want_coll, dispatch=disp, **dict(run, **(constants or {})))
        env.reset()
        st = env.get_state()
        env.set_state(st['pos'] * 0.3, st['vel'], st['landmarks'], ep_step=as_clocks(clocks),   # crowded: contacts in most steps
                      ep_count=st['ep_count'] if ep_count is None else torch.as_tensor(ep_count).int().cuda())
        outs = []
        for i, a in enumerate(acts):
            if reclock and i in reclock:
                st = env.get_state()
                env.set_state(st['pos'], st['vel'], st['landmarks'], ep_step=as_clocks(reclock[i]), ep_count=st['ep_count'])
            o = env.rollout(a.cuda())
            outs.append({k: v.clone() for k, v in o.items()})
            if ep_len > 1:   # (episodes of one step: the host sends every multi-wave form to the one-wave kernel)
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


def _terminal(outs):
    return torch.cat([o['terminal'].bool() for o in outs])


def _saw_a_reset(outs):
    term = _terminal(outs)
    assert term.any() and not term.all()


@pytest.mark.parametrize('B', [4, 8, 13, 20])
@pytest.mark.parametrize('launches', [(12,), (13,), (40,), (5, 20), (11, 1, 12)], ids=SEQ_IDS)
def test_synchronised_clocks(B, launches):
    """Episodes of 12 steps, every clock at 0.  (12,): the launch ends in the reset step; (13,): one step behind it; (40,): three episode
    ends in one launch, the second and third served by pipelines that started behind a reset step; (5, 20): the pipeline of the second
    launch starts in mid-episode; (11, 1, 12): a launch that is the reset step alone (T = 1).  B = 4: the second physics wave idles;
    8: one full workgroup; 13: a partial last workgroup; 20: two and a half workgroups.  Seeded uniform indices, then the ramp."""
    for acts in (_uniform(B, launches), _ramp(B, launches)):
        outs = _check(_both(B, acts))
        _saw_a_reset(outs)
        assert bool(_terminal(outs)[EP - 1].all())   # every env ends its episode in the same step


@pytest.mark.parametrize('k', [EP - D - 1, EP - D, EP - D + 1])
def test_resets_around_the_depth(k):
    """Launches (k, 12): the second launch's first reset falls in its step 11 - k = D, D - 1, D - 2 -- the first step that may use the
    draws, and the two before it, which may not."""
    assert k >= 1
    for B in (8, 13):
        outs = _check(_both(B, _uniform(B, (k, EP))))
        assert bool(outs[1]['terminal'].bool()[EP - 1 - k].all()) and not bool(outs[0]['terminal'].bool().any())
    _check(_both(13, _ramp(13, (k, EP))))


@pytest.mark.parametrize('ep_len', sorted({1, 2, 3, D - 1, D, D + 1, D + 2, 25} - {0}))
def test_episode_lengths(ep_len):
    """Up to D steps the pipeline never engages (and the reset steps of the shortest episodes come in consecutive iterations); D + 1 is
    the shortest episode that is served from it."""
    for B, acts in ((13, _uniform(13, (40,))), (20, _ramp(20, (7, 33)))):
        outs = _check(_both(B, acts, ep_len=ep_len))
        term = _terminal(outs)
        assert term.any() and (ep_len == 1 or not term.all())


def test_clocks_equal_inside_a_workgroup_and_different_between_workgroups():
    """B = 20, clocks 0, 5, 9 per block of 8: every workgroup takes the fast path, each at a step of its own."""
    clocks = [0] * 8 + [5] * 8 + [9] * 4
    for acts in (_uniform(20, (40,)), _ramp(20, (5, 20))):
        outs = _check(_both(20, acts, clocks=clocks))
        term = _terminal(outs)
        assert bool(term[EP - 1, :8].all()) and bool(term[EP - 6, 8:16].all()) and bool(term[EP - 10, 16:].all())
        assert not bool(term[EP - 1, 8:].any())


def test_clocks_apart_inside_a_workgroup():
    """One env of each workgroup one step ahead of the others: the code as it was before, throughout."""
    for B in (8, 13):
        clocks = [0] * B
        clocks[3] = 1
        clocks[B - 1] = 1
        outs = _check(_both(B, _uniform(B, (40,)), clocks=clocks))
        term = _terminal(outs)
        assert bool(term[EP - 2, 3]) and not bool(term[EP - 2, 0]) and bool(term[EP - 1, 0])


def test_desynchronised_then_synchronised():
    """Clocks apart for one launch, then set equal (set_state) for the next launch on the same handle; and the other way round."""
    B = 13
    apart = ((torch.arange(B) * 7) % EP).tolist()
    outs = _check(_both(B, _uniform(B, (17, 30)), clocks=apart, reclock={1: 2}))
    assert bool(outs[1]['terminal'].bool()[EP - 3].all())
    _saw_a_reset(outs)
    outs = _check(_both(B, _uniform(B, (17, 30)), clocks=0, reclock={1: apart}))
    _saw_a_reset(outs)


@pytest.mark.parametrize('env_id_base', [0, 1000, (1 << 32) - 5, (1 << 32) + 5], ids=['0', '1000', '2^32-5', '2^32+5'])
def test_per_env_episode_counts_and_env_ids(env_id_base):
    """The draw's counter words are the lane's own: episode counts that differ per env (one of them about to wrap), a nonzero first env
    id, one whose low word carries into the high one inside the batch, and one above 2^32 (the id's high word)."""
    B = 13
    counts = ((torch.arange(B) * 3 + 1) % 11).tolist()
    counts[5] = -2   # 0xFFFFFFFE as the state's int32: the next two episodes are 0xFFFFFFFF and 0
    outs = _check(_both(B, _uniform(B, (40,)), ep_count=counts, env_id_base=env_id_base))
    _saw_a_reset(outs)


def test_env_ids_reach_the_draws():
    B = 8
    a = _both(B, _uniform(B, (14,)))['quad'][1]
    b = _both(B, _uniform(B, (14,)), env_id_base=1000)['quad'][1]
    assert not torch.equal(a['pos'], b['pos']) and not torch.equal(a['landmarks'], b['landmarks'])


def test_the_collision_mask_instantiation():
    for B in (8, 13):
        outs = _check(_both(B, _uniform(B, (40,)), want_coll=True), want_coll=True)
        _saw_a_reset(outs)


def test_the_unit_world():
    """tests/world_constants.py `unit`: unit mass (the quad kernel needs it), a force table of its own."""
    for B in (8, 13):
        outs = _check(_both(B, _ramp(B, (40,)), want_coll=True, world='unit'), want_coll=True)
        _saw_a_reset(outs)


def test_a_margin_that_needs_the_full_division():
    """A contact margin whose significand is all ones: the host's margin test (pw_margin_one_correction) fails, K1 is false."""
    from multiagent_rl_amd import _lib
    margin = float(np.float32(0.0009765624417923391))
    assert _lib.load().pw_margin_one_correction(C.c_float(margin)) == 0
    for want_coll in (False, True):
        outs = _check(_both(13, _uniform(13, (40,)), want_coll=want_coll, constants=dict(contact_margin=margin)), want_coll=want_coll)
        _saw_a_reset(outs)
