"""pw_spread_quad_kernel's instruction-stream diet (running plane pointers, wave OB's straight-line step, the physics waves' folded
near / range test with its cold block, the action fetch from a running scalar base): every output and the state after the launch
equal the one-wave stream kernel's bit for bit, at the smallest shapes at which the rewritten code can go wrong.  A CPU test reads
the loop structure off the built object (tools/loop_census.py)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import code_object  # noqa: E402

torch = pytest.importorskip('torch')

AUTO = dict(force_generic=0, no_stream=0, duo=-1, quad=-1, obs_block=-1, trio=-1, p_prio=-1, envs_per_wave=0, policy_form=0)
N = 6
OUTS = ('obs', 'rew', 'rew_shared', 'done', 'terminal')
STATE = ('pos', 'vel', 'landmarks', 'ep_step', 'ep_count')


def _same(a, b, name):
    """Bitwise, by the suite's rule (tests/test_gpu_parity.py _assert_same_bits): float tensors are compared as their int32 patterns,
    and a NaN equals a NaN.  The sign and payload of a NaN are no output of the environment, and the pair-parallel physics cannot
    share them with the per-agent kernels: a pair's second agent receives the NEGATED force, so where that force is NaN (0 / 0 between
    coincident agents) its sign bit is the opposite of the one the stream kernel computes from that agent's own side."""
    assert a.shape == b.shape and a.dtype == b.dtype, (name, a.shape, b.shape, a.dtype, b.dtype)
    if a.dtype.is_floating_point:
        same = (a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)) | (torch.isnan(a) & torch.isnan(b))
        assert bool(same.all()), (name, int((~same).sum()))
    else:
        assert torch.equal(a, b), name


def _both(B, launches, ep_len=25, want_coll=False, edit_state=None, desync=True, quad_required=True, **world):
    """The same start state and actions through the stream kernel and the quad kernel, `launches` (a tuple of step counts)
    consecutive rollouts into one handle each.  -> {form: ([outputs per launch], state after)}"""
    from multiagent_rl_amd.env import BatchedParticleEnv
    gen = torch.Generator().manual_seed(1000 * B + sum(launches))
    acts = [torch.randint(0, 5, (T, B, N), dtype=torch.int32, generator=gen).cuda() for T in launches]
    res = {}
    for form, disp, kernel in (('stream', dict(AUTO, duo=0), 'pw_spread_stream_kernel'), ('quad', dict(AUTO, quad=1), 'pw_spread_quad_kernel')):
        env = BatchedParticleEnv('simple_spread', B, num_agents=N, max_episode_len=ep_len, auto_reset=True, seed=41, want_coll=want_coll,
                                 dispatch=disp, **world)
        env.reset()
        st = env.get_state()
        pos = st['pos'] * 0.3   # crowded: contacts in most steps
        if edit_state is not None:
            pos = edit_state(pos.clone())
        ep_step = ((torch.arange(B, device='cuda') * 7) % ep_len).int() if desync else st['ep_step']
        env.set_state(pos, st['vel'], st['landmarks'], ep_step=ep_step, ep_count=st['ep_count'])
        outs = []
        for a in acts:
            o = env.rollout(a)
            outs.append({k: v.clone() for k, v in o.items()})
            assert env.last_kernel().startswith(kernel) or not quad_required, env.last_kernel()
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


@pytest.mark.gpu
@pytest.mark.parametrize('B', [8, 13, 3])
@pytest.mark.parametrize('T', [1, 2, 3, 5, 9])
def test_quad_equals_stream_at_small_batches_and_short_launches(B, T):
    """B = 8: one full workgroup; 13: a full one and one of 5 envs (the second physics wave has one env, 18 of wave OB's 48 rows are
    past the block); 3: the second physics wave has none.  T below the action fetch depth of four runs on the clamped tail, T = 1
    is wave OA's prologue and epilogue around an empty loop.  Episodes of 3 steps with desynchronised clocks: resets in most steps."""
    outs = _check(_both(B, (T,), ep_len=3))
    assert T < 3 or outs[0]['terminal'].any()


@pytest.mark.gpu
@pytest.mark.parametrize('ep_len', [2, 3, 25])
def test_quad_equals_stream_with_desynchronised_episode_clocks(ep_len):
    """Reset steps in consecutive iterations, a second ring slot in most steps (episodes of 2 and 3), and the common no-reset path
    between resets (25), with the collision masks: the `quad+coll` instantiation."""
    outs = _check(_both(13, (31,), ep_len=ep_len, want_coll=True), want_coll=True)
    term = outs[0]['terminal'].bool()
    assert term.any() and not term.all()


@pytest.mark.gpu
def test_two_launches_into_one_handle_restart_the_running_pointers():
    """T = 5 then T = 9 into the same handle: the plane pointers start from each launch's own buffers, the state carries over."""
    _check(_both(13, (5, 9), ep_len=3))


@pytest.mark.gpu
@pytest.mark.parametrize('world, kernel', [
    (dict(contact_margin=float(np.float32(0.0009765624417923391))), 'pw_spread_quad_kernel<true,true>'),   # a significand of all ones: K1 false
    # the dispatcher launches the quad kernel at unit mass only (pworld.hip quad_ok): a forced quad=1 with another mass must still
    # compute what the stream kernel does, through whichever kernel it falls back to
    (dict(mass=2.0), 'pw_spread_'),
], ids=['margin', 'mass'])
def test_the_other_instantiations_run_the_new_code_too(world, kernel):
    res = _both(13, (9,), ep_len=3, want_coll='contact_margin' in world, quad_required='mass' not in world, **world)
    assert res['quad'][2].startswith(kernel), res['quad'][2]
    if 'mass' in world:
        assert 'quad' not in res['quad'][2]
    _check(res, want_coll='contact_margin' in world)


def _coincident(pos):
    pos[2, 1] = pos[2, 0]   # env 2: agents 0 and 1 at the same point -- d2 = 0, near and out of the fast range
    return pos


def _nan(pos):
    pos[5, 3, 0] = float('nan')
    return pos


@pytest.mark.gpu
@pytest.mark.parametrize('edit', [_coincident, _nan], ids=['coincident', 'nan'])
def test_the_cold_force_path_equals_stream(edit):
    """Coincident agents (dist = 0: the general expressions divide by it) and a NaN coordinate take the physics waves' out-of-line
    block; B = 8, the other seven envs stay on the fast path in the same waves.  No reset in the launch: the states persist."""
    res = _both(8, (5,), ep_len=25, edit_state=edit, desync=False)
    outs = _check(res)
    assert not torch.isfinite(outs[0]['obs']).all()   # the exceptional values did reach the outputs


@pytest.mark.skipif(not code_object.tools_present(), reason='ROCm LLVM binary tools not installed')
def test_quad_kernel_loop_structure():
    """Structure only (the counts are recorded in profiles/r6_quad_loop_census.txt, not asserted): the kernel's loops that hold a
    barrier are exactly the three step loops and the idle physics wave's, and a common step of wave OB has no exec-masked branch."""
    import loop_census
    from multiagent_rl_amd import build_native
    if not all(os.path.exists(o) for o in build_native.objects()):
        build_native.build(force=True)
    for inst in ('pw_spread_quad_kernel<true,false,true>', 'pw_spread_quad_kernel<true,true,false>'):
        _, loops = loop_census.kernel_loops(inst)
        steps = [lp for lp in loops if lp['role']]
        assert sorted(lp['role'] for lp in steps) == ['OA', 'OB', 'P', 'idle'], [lp['role'] for lp in steps]
        ob = [lp for lp in steps if lp['role'] == 'OB'][0]
        assert ob['common_ops'] and not [o for o in ob['common_ops'] if o.startswith('s_cbranch_exec')], ob['common_ops']
