"""GPU: non-finite inputs through the network kernels -- the dense front, the LSTM recurrence, attention pooling, the Gumbel sample, the
no-gradient critics, every actor form, the one-launch policy rollouts and one update of the example learner.

The environment half treats NaN as part of its contract (two coincident agents give 0 / 0, and the kernels carry that NaN like upstream);
a rollout writes such rows into the ring and the learner samples them.  Three criteria (tests/nonfinite.py), throughout:

(M) ``~isfinite`` of the kernel's tensor equals ``~isfinite`` of the float64 restatement's, elementwise;
(I) every row-local output of every clean row is bit-identical to the same launch on the clean inputs;
(R) every action index of a poisoned row lies in [0, n).

The float64 restatements are checked against float64 autograd of the stock expressions in tests/test_nonfinite_host.py.  Values inside
poisoned rows are not compared.  The poison is NaN; +Inf in addition where a case says so.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

from oracle import actor_oracle as ao  # noqa: E402  (checker only)
from oracle import c_oracle as co  # noqa: E402
from tests import attention_ref, dense_ref, lstm_ref, nonfinite as nf, sampling_ref  # noqa: E402


def _cuda(v):
    if v is None:
        return None
    if isinstance(v, (tuple, list)):
        return [_cuda(t) for t in v]
    return (torch.from_numpy(v) if isinstance(v, np.ndarray) else v).cuda()


# ---- the dense front ---------------------------------------------------------------------------------------------------------------
def _dense_launch(inp, dG):
    """One forward and one backward (both dx requested) -> dict of everything they return."""
    from multiagent_rl_amd import dense
    a = {k: _cuda(v) for k, v in inp.items()}
    G, hid = dense.launch_forward(a['x0'], a['x1'], a['w1'], a['b1'], a['w_ih'], a['b_ih'], a['b_hh'], True)
    dW1, db1, dW_ih, db_gate, dx0, dx1 = dense.launch_backward(dG.cuda(), a['x0'], a['x1'], hid, a['w1'], a['w_ih'], True, True)
    out = dict(hid=hid, G=G, dx0=dx0, dx1=dx1, dW1=dW1, db1=db1)
    for d in range(len(dW_ih)):
        out['dW_ih%d' % d], out['db_gate%d' % d] = dW_ih[d], db_gate[d]
    return out


def _dense_reference(inp, dG):
    """float64: hid, G and dx from the restatement, the parameter gradients from autograd of the stock expression."""
    f = nf.dense_f64(inp)
    hid, G = dense_ref.forward(**f)
    ours = dense_ref.backward(dG.double(), f['x0'], f['x1'], hid, f['w1'], f['w_ih'])
    _, stock = dense_ref.stock_grads(lambda g: (g * dG.double()).sum(), **f)
    ref = dict(hid=hid, G=G, dx0=ours['dx0'], dx1=ours['dx1'], dW1=stock['dW1'], db1=stock['db1'])
    for d in range(len(f['w_ih'])):
        ref['dW_ih%d' % d], ref['db_gate%d' % d] = stock['dW_ih%d' % d], stock['db_gate%d' % d]
    return ref


def _dense_case(d0, d1, dirs, which, col, r, value, clean):
    inp, dG = nf.dense_inputs(d0, d1, dirs)
    bad = dict(inp, **{which: nf.poisoned(inp[which], (r, col), value)})
    tag = 'dense d0 %d d1 %d dirs %d %s[%d, %d] = %r' % (d0, d1, dirs, which, r, col, value)
    got, ref = _dense_launch(bad, dG), _dense_reference(bad, dG)
    for n in ref:
        nf.assert_same_mask(got[n], ref[n], tag + ' ' + n)
    for n in ('hid', 'G', 'dx0', 'dx1'):
        nf.assert_clean_rows_same_bits(got[n], clean[n], [r], tag + ' ' + n)
    k = col if which == 'x0' else d0 + col
    m = nf.nonfinite(got['dW1'])
    assert list(nf.rows_with(m, axis=1)) == [k] and m[:, k].all(), tag + ': exactly one column of dW1'
    assert nf.nonfinite(got['G'])[r].all() and (value == value or nf.nonfinite(got['hid'])[r].all()), tag
    return got


@pytest.mark.parametrize('d0,d1,dirs', nf.DENSE_SHAPES)
def test_dense_front_carries_a_nan_row_and_nothing_else(d0, d1, dirs):
    inp, dG = nf.dense_inputs(d0, d1, dirs)
    clean = _dense_launch(inp, dG)
    assert all(bool(torch.isfinite(t).all()) for t in clean.values())
    for which, col in nf.dense_poisons(d0, d1):
        for r in nf.rows_to_poison(nf.DENSE_ROWS):
            got = _dense_case(d0, d1, dirs, which, col, r, nf.NAN, clean)
            for d in range(dirs):                                  # every hidden unit of the row is NaN: dW_ih = dG^T hid is NaN everywhere
                assert nf.nonfinite(got['dW_ih%d' % d]).all(), (which, r, d)


def test_dense_front_carries_an_infinite_observation():
    """x0[r, 3] = +Inf: hid is +Inf or 0 by the sign of the weight, G mixes both signs; the masks are still the float64 ones."""
    d0, d1, dirs = nf.DENSE_SHAPES[1]
    inp, dG = nf.dense_inputs(d0, d1, dirs)
    _dense_case(d0, d1, dirs, 'x0', 3, nf.rows_to_poison(nf.DENSE_ROWS)[1], nf.INF, _dense_launch(inp, dG))


# ---- the LSTM recurrence -----------------------------------------------------------------------------------------------------------
def _lstm_launch(G, w_fw, w_bw, dY):
    from multiagent_rl_amd import lstm
    w_fw, w_bw = _cuda(w_fw), _cuda(w_bw)
    Y, saved = lstm.launch_forward(G.cuda(), w_fw, w_bw, True)
    return dict(Y=Y, saved=saved, dG=lstm.launch_backward(dY.cuda(), saved, w_fw, w_bw))


def _lstm_reference(G, w_fw, w_bw, dY):
    w_fw, w_bw = w_fw.double(), None if w_bw is None else w_bw.double()
    Y, saved = lstm_ref.forward(G.double(), w_fw, w_bw)
    return dict(Y=Y, saved=saved, dG=lstm_ref.backward(dY.double(), saved, w_fw, w_bw))


@pytest.mark.parametrize('dirs,H', nf.LSTM_SHAPES)
def test_lstm_recurrence_carries_a_nan_gate_forward_in_its_direction_only(dirs, H):
    G, w_fw, w_bw, dY = nf.lstm_inputs(dirs, H)
    clean = _lstm_launch(G, w_fw, w_bw, dY)
    assert all(bool(torch.isfinite(t).all()) for t in clean.values())
    t, d, col = nf.LSTM_POISON
    for r in nf.rows_to_poison(nf.LSTM_B):
        bad = nf.poisoned(G, (r, t, d, col))
        got, ref = _lstm_launch(bad, w_fw, w_bw, dY), _lstm_reference(bad, w_fw, w_bw, dY)
        for n in ref:                                              # per step and per direction: the reference's mask says which
            nf.assert_same_mask(got[n], ref[n], 'lstm dirs %d H %d G[%d, %d, %d, %d] %s' % (dirs, H, r, t, d, col, n))
            nf.assert_clean_rows_same_bits(got[n], clean[n], [r], 'lstm dirs %d H %d row %d %s' % (dirs, H, r, n))
        m = nf.nonfinite(got['Y']).reshape(nf.LSTM_B, nf.LSTM_N, dirs, H)
        assert not m[r, :t].any() and m[r, t + 1:, 0].all() and not m[r, :, 1:].any()
        # the other direction of the poisoned row is a row-local output of a clean sequence: its bits too
        if dirs == 2:
            for n in ('Y', 'saved', 'dG'):
                g = got[n].reshape(nf.LSTM_B, nf.LSTM_N, dirs, -1)[:, :, 1].contiguous()
                c = clean[n].reshape(nf.LSTM_B, nf.LSTM_N, dirs, -1)[:, :, 1].contiguous()
                nf.assert_clean_rows_same_bits(g, c, [], 'lstm direction 1 of row %d %s' % (r, n))


@pytest.mark.parametrize('dirs,H', nf.LSTM_SHAPES)
def test_lstm_recurrence_saturates_on_an_infinite_gate(dirs, H):
    G, w_fw, w_bw, dY = nf.lstm_inputs(dirs, H)
    t, d, col = nf.LSTM_POISON
    r = nf.rows_to_poison(nf.LSTM_B)[1]
    bad = nf.poisoned(G, (r, t, d, col), nf.INF)
    got, ref, clean = _lstm_launch(bad, w_fw, w_bw, dY), _lstm_reference(bad, w_fw, w_bw, dY), _lstm_launch(G, w_fw, w_bw, dY)
    for n in ref:
        assert not nf.nonfinite(ref[n]).any() and not nf.nonfinite(got[n]).any(), n
        nf.assert_clean_rows_same_bits(got[n], clean[n], [r], 'lstm +inf ' + n)
    assert float(got['saved'][r, t, d, 0, col]) == 1.0              # the input gate of that unit: sigmoid(+Inf)


# ---- attention pooling -------------------------------------------------------------------------------------------------------------
def _attention_launch(Y, dOut, relu):
    from multiagent_rl_amd import attention
    Y = Y.cuda()
    out, weight = attention.launch_forward(Y, relu, True)
    return dict(out=out, weight=weight, dY=attention.launch_backward(dOut.cuda(), Y, weight, out, relu))


def _attention_reference(Y, dOut, relu):
    out, weight = attention_ref.forward(Y.double(), relu)
    return dict(out=out, weight=weight, dY=attention_ref.backward(dOut.double(), Y.double(), weight, out, relu))


@pytest.mark.parametrize('relu', [True, False], ids=['relu', 'norelu'])
@pytest.mark.parametrize('b,N', nf.ATTENTION_SHAPES)
def test_attention_pool_carries_a_nan_row_and_nothing_else(b, N, relu):
    Y, dOut = nf.attention_inputs(b, N)
    clean = _attention_launch(Y, dOut, relu)
    assert all(bool(torch.isfinite(t).all()) for t in clean.values())
    for step in nf.attention_poisons(N):
        for r in nf.rows_to_poison(b):
            bad = nf.poisoned(Y, (r, step, nf.ATTENTION_COLUMN))
            got, ref = _attention_launch(bad, dOut, relu), _attention_reference(bad, dOut, relu)
            for n in ref:
                tag = 'attention b %d N %d relu %d Y[%d, %d, %d] %s' % (b, N, relu, r, step, nf.ATTENTION_COLUMN, n)
                nf.assert_same_mask(got[n], ref[n], tag)
                nf.assert_clean_rows_same_bits(got[n], clean[n], [r], tag)
            assert nf.nonfinite(got['out'])[r].all()


# ---- the Gumbel sample -------------------------------------------------------------------------------------------------------------
def _sample_launch(logits, dY, hard, soft=None):
    """The forward (y, soft, idx) and the backward on its own ``soft`` (or on ``soft`` given)."""
    from multiagent_rl_amd import sampling
    y, s, idx, _ = sampling.launch_forward(logits.cuda(), nf.SAMPLE_TAU, hard, nf.SAMPLE_SEED, nf.SAMPLE_STEP, None, True, want_idx=True)
    return dict(y=y, soft=s, idx=idx, dLogits=sampling.launch_backward(dY.cuda(), s if soft is None else soft, nf.SAMPLE_TAU))


def _sample_reference(logits, dY, hard, n, soft=None):
    nz = sampling_ref.noise(nf.SAMPLE_SEED, nf.SAMPLE_STEP, nf.SAMPLE_ROWS, n)
    y, s, _ = sampling_ref.forward(logits.double(), nz, nf.SAMPLE_TAU, hard)
    return dict(y=y, soft=s, dLogits=sampling_ref.backward(dY.double(), s if soft is None else soft, nf.SAMPLE_TAU))


@pytest.mark.parametrize('hard', [True, False], ids=['hard', 'soft'])
@pytest.mark.parametrize('n', nf.SAMPLE_WIDTHS)
def test_gumbel_sample_carries_a_nan_row_and_keeps_its_index_in_range(n, hard):
    logits, dY = nf.sample_inputs(n)
    clean = _sample_launch(logits, dY, hard)
    assert all(bool(torch.isfinite(t.float()).all()) for t in clean.values())
    soft64 = _sample_reference(logits, dY, hard, n)['soft']
    for r in nf.rows_to_poison(nf.SAMPLE_ROWS):
        for col in (0, n - 1):
            bad = nf.poisoned(logits, (r, col))
            got, ref = _sample_launch(bad, dY, hard), _sample_reference(bad, dY, hard, n)
            for name in ref:
                tag = 'sample n %d hard %d logits[%d, %d] %s' % (n, hard, r, col, name)
                nf.assert_same_mask(got[name], ref[name], tag)
                nf.assert_clean_rows_same_bits(got[name], clean[name], [r], tag)
            nf.assert_clean_rows_same_bits(got['idx'], clean['idx'], [r], 'sample idx')
            nf.assert_in_range(got['idx'], n, 'sample n %d hard %d logits[%d, %d] idx' % (n, hard, r, col))
            assert nf.nonfinite(got['y'])[r].all() and nf.nonfinite(got['soft'])[r].all()
        # the backward's own poison: one element of dY, on the clean forward's soft
        bad_dY = nf.poisoned(dY, (r, 2))
        got = _sample_launch(logits, bad_dY, hard, soft=clean['soft'])['dLogits']
        ref = _sample_reference(logits, bad_dY, hard, n, soft=soft64)['dLogits']
        nf.assert_same_mask(got, ref, 'sample n %d hard %d dY[%d, 2]' % (n, hard, r))
        nf.assert_clean_rows_same_bits(got, clean['dLogits'], [r], 'sample n %d hard %d dY[%d, 2]' % (n, hard, r))


# ---- the no-gradient critics -------------------------------------------------------------------------------------------------------
def _critic_launch(fc, form, obs, next_obs, inp):
    """q (and the model head's r) on ``obs``, the TD target on ``next_obs``."""
    act = _cuda(inp['act'])
    out = dict(q=fc.q(_cuda(obs), act))
    if form == 'model':
        out['r'] = fc.reward(_cuda(obs), act)
    out['y'], out['q_next'] = fc.td_target(_cuda(next_obs), act, _cuda(inp['rew']), _cuda(inp['done']), nf.CRITIC_GAMMA, return_q=True)
    return out


def _critic_reference(net, form, obs, next_obs, inp):
    out = nf.critic_f64(form, net, obs, inp['act'])
    out['q_next'] = nf.critic_f64(form, net, next_obs, inp['act'])['q']
    out['y'] = inp['rew'].astype(np.float64) + nf.CRITIC_GAMMA * out['q_next'] * (1.0 - inp['done'].astype(np.float64))
    return out


@pytest.mark.parametrize('form', nf.CRITIC_FORMS)
def test_critic_forward_and_td_target_carry_a_nan_row_and_nothing_else(form):
    from multiagent_rl_amd.critic import FusedCritic
    net = nf.critic_net(form).cuda()
    fc = FusedCritic(net)
    assert (fc.per_step, fc.model) == (form == 'bicnet', form == 'model')
    inp = nf.critic_inputs(form)
    clean = _critic_launch(fc, form, inp['obs'], inp['next_obs'], inp)
    assert all(bool(torch.isfinite(t).all()) for t in clean.values())
    agent, col = nf.CRITIC_POISON
    for r in nf.rows_to_poison(nf.CRITIC_B):
        for which in ('obs', 'next_obs'):
            both = dict(obs=inp['obs'], next_obs=inp['next_obs'])
            both[which] = nf.poisoned(inp[which], (r, agent, col))
            got, ref = _critic_launch(fc, form, both['obs'], both['next_obs'], inp), _critic_reference(net, form, both['obs'], both['next_obs'], inp)
            for n in ref:
                tag = '%s critic %s[%d, %d, %d] %s' % (form, which, r, agent, col, n)
                nf.assert_same_mask(got[n], ref[n], tag)
                nf.assert_clean_rows_same_bits(got[n], clean[n], [r], tag)
            hit = ('q', 'r') if which == 'obs' else ('q_next', 'y')
            for n in ref:
                assert nf.nonfinite(got[n]).any() == (n in hit), (form, which, r, n)
            if form == 'bicnet':                                   # per step: finite before the poisoned agent
                assert list(nf.nonfinite(got[hit[0]])[r]) == [False, True, True]


# ---- the actor ---------------------------------------------------------------------------------------------------------------------
def _actor_launch(fused, obs, call=7):
    x = _cuda(obs)
    lg = fused.logits(x)
    fused.calls = call                                              # the same noise in every launch compared
    return dict(H=fused.hidden(x), logits=torch.cat(lg, -1) if isinstance(lg, list) else lg, act=fused(x))


@pytest.mark.parametrize('form', list(nf.ACTOR_FORMS))
def test_actor_carries_a_nan_env_and_nothing_else(monkeypatch, form):
    """One-launch actor16, the three-launch chain, one wide-row shape (D > 64: pw_actor_fused_kernel) and the bf16x3 input projection."""
    from multiagent_rl_amd import _lib
    from multiagent_rl_amd.policy import ActorNetwork, FusedActor
    D = nf.ACTOR_FORMS[form]
    torch.manual_seed(D)
    net = ActorNetwork(D, nf.ACTOR_LOGITS).cuda().eval()
    if form == 'chain':
        monkeypatch.setenv('PW_ACTOR_NO_FUSE', '1')
    fused = FusedActor(net, seed=9)
    assert fused.use_fused == (form != 'chain')
    lib = _lib.load()
    prev = lib.pw_actor_set_bf16x3(1) if form == 'bf16x3' else None
    try:
        obs = nf.actor_obs(D)
        clean = _actor_launch(fused, obs)
        assert all(bool(torch.isfinite(t.float()).all()) for t in clean.values())
        agent, col = nf.ACTOR_POISON
        for env in nf.ACTOR_ENVS:
            bad = nf.poisoned(obs, (env, agent, col))
            got = _actor_launch(fused, bad)
            H64, lg64 = ao.forward_f64(net, bad)
            tag = 'actor %s obs[%d, %d, %d]' % (form, env, agent, col)
            nf.assert_same_mask(got['H'], H64, tag + ' H')          # the BiLSTM spreads it over the env's agents: the oracle's mask says how
            nf.assert_same_mask(got['logits'], np.concatenate(lg64, -1), tag + ' logits')
            assert list(nf.rows_with(nf.nonfinite(got['logits']))) == [env] and nf.nonfinite(got['logits'])[env].all()
            for n in ('H', 'logits', 'act'):
                nf.assert_clean_rows_same_bits(got[n], clean[n], [env], tag + ' ' + n)
            nf.assert_in_range(got['act'][env], nf.ACTOR_LOGITS, tag + ' act')
    finally:
        if prev is not None:
            lib.pw_actor_set_bf16x3(prev)


# ---- the one-launch policy rollouts: the environment produces the NaN --------------------------------------------------------------
ROLL_B, ROLL_N, ROLL_T, ROLL_LEN, ROLL_ENVS = 19, 3, 12, 5, (5, 17)
ROLLOUTS = {   # name -> (scenario, env kwargs, oracle kwargs, policy_form, kernel)
    'form3': ('simple_spread', dict(n=ROLL_N), {}, 3, 'pw_policy_rollout3_kernel'),
    'form3j': ('simple_spread', dict(n=ROLL_N), {}, 4, 'pw_policy_rollout3j_kernel'),
    'generic': ('simple_spread', dict(n=ROLL_N), {}, 5, 'pw_policy_rollout_generic_kernel'),
    'tag2+1': ('simple_tag', dict(num_adversaries=2, num_good=1), dict(num_adversaries=2), 0, 'pw_policy_rollout_tag_kernel'),
}
ROLL_KEYS = ('obs', 'rew', 'act', 'terminal')


def _roll_env(name):
    from multiagent_rl_amd import make_batched_env
    scenario, kw, okw, form, _ = ROLLOUTS[name]
    env = make_batched_env(scenario, ROLL_B, auto_reset=True, max_episode_len=ROLL_LEN, seed=21, **kw)
    if form:
        env.set_dispatch(policy_form=form)
    cfg = co.make_config(scenario, ROLL_N, max_episode_len=ROLL_LEN, auto_reset=True, seed=21, **okw)
    return env, co.COracle(cfg, ROLL_B, np.float32)


def _roll_start(name, coincide):
    """-> (env, oracle, the rows the policy sees first): after the keyed reset; ``coincide``: agents 0 and 1 of ROLL_ENVS on one point."""
    from tests.test_gpu_parity import _assert_same_bits, _np
    env, o32 = _roll_env(name)
    _assert_same_bits(_np(env.reset()), o32.reset(), 'reset obs')
    if coincide:
        pos = o32.pos.copy()
        for e in ROLL_ENVS:
            pos[e, 1] = pos[e, 0]
        env.set_state(pos, o32.vel.copy(), o32.lm.copy())
        o32.set_state(pos, o32.vel.copy(), o32.lm.copy())
        _assert_same_bits(_np(env.observe()), o32.observe(), 'obs after set_state')
    obs0 = o32.observe()
    assert np.isfinite(obs0).all()                                  # coincident, not yet NaN: the first step divides 0 by 0
    return env, o32, obs0


@pytest.mark.parametrize('name', list(ROLLOUTS))
def test_policy_rollout_keeps_a_nan_env_to_itself(name):
    from multiagent_rl_amd.policy import ActorNetwork, FusedActor
    from tests.test_gpu_actor_reference import assert_rollout_actions_match_f64
    from tests.test_gpu_parity import _assert_same_bits, _np
    from tests.test_gpu_policy_oracle import _replay_through_oracle
    T, B, N = ROLL_T, ROLL_B, ROLL_N
    others = np.setdiff1d(np.arange(B), ROLL_ENVS)
    torch.manual_seed(4)
    env, o32, obs0 = _roll_start(name, True)
    net = ActorNetwork(env.obs_dim, 5).cuda().eval()
    got = FusedActor(net, seed=9).rollout(env, T)
    assert env.last_kernel().startswith(ROLLOUTS[name][4]), env.last_kernel()
    out = {k: _np(got[k]) for k in ROLL_KEYS}
    # 1. every environment output equals the float32 oracle on the launch's own actions (NaN counts as equal to NaN)
    assert _replay_through_oracle(o32, got, T) == T // ROLL_LEN
    first_reset = ROLL_LEN - 1                                      # the step whose outputs are the first post-reset ones
    assert out['terminal'][first_reset].all() and not out['terminal'][:first_reset].any()
    for e in ROLL_ENVS:                                             # the coincidence did what it is there for
        assert np.isnan(out['obs'][:first_reset, e]).any(axis=(1, 2)).all()
    # 2. every other env, every step: the bits of a run from the same state without the coincidence
    env_c, _, obs0_c = _roll_start(name, False)
    clean = {k: _np(v) for k, v in FusedActor(net, seed=9).rollout(env_c, T).items() if k in ROLL_KEYS}
    assert all(np.isfinite(clean[k].astype(np.float64)).all() for k in ROLL_KEYS)
    for k in ROLL_KEYS:
        nf.assert_clean_rows_same_bits(out[k], clean[k], ROLL_ENVS, '%s %s' % (name, k), axis=1)
    # 3. from their first reset on the poisoned envs are the clean run's too: the reset draw and the noise are keyed, not stateful
    for e in ROLL_ENVS:
        _assert_same_bits(out['obs'][first_reset:, e], clean['obs'][first_reset:, e], 'obs of env %d after its reset' % e)
        for k in ('rew', 'act'):
            _assert_same_bits(out[k][first_reset + 1:, e], clean[k][first_reset + 1:, e], '%s of env %d after its reset' % (k, e))
        assert np.isfinite(out['obs'][first_reset:, e]).all()
    # 4. the poisoned envs' actions stay inside the force table
    nf.assert_in_range(out['act'][:, list(ROLL_ENVS)], 5, name + ' act')
    # 5. the per-step loop from the same start: the same bits
    env_l = _roll_start(name, True)[0]
    loop = FusedActor(net, seed=9)
    obs = env_l.observe()
    for t in range(T):
        act = loop(obs)
        obs, rew, _, info = env_l.step(act)
        assert np.array_equal(_np(act), out['act'][t]), 'act[%d]' % t
        _assert_same_bits(_np(obs), out['obs'][t], 'loop obs[%d]' % t)
        _assert_same_bits(_np(rew), out['rew'][t], 'loop rew[%d]' % t)
        assert np.array_equal(_np(info['terminal']).astype(np.uint8), out['terminal'][t].astype(np.uint8))
    # 6. the actions against the float64 actor on the clean rows; the rows left out are exactly those whose float64 logits are NaN
    rows = np.concatenate([obs0[None], out['obs'][:-1]], 0)
    P = ao.actor_params(net)
    nan_logits = np.stack([np.isnan(ao.forward_f64(P, rows[t])[1][0]).any(axis=(1, 2)) for t in range(T)])        # [T, B]
    want = np.zeros((T, B), bool)
    want[1:first_reset + 1, list(ROLL_ENVS)] = True                 # the rows of steps 0 .. first_reset - 1 are seen one step later
    assert np.array_equal(nan_logits, want) and int(nan_logits.sum()) == len(ROLL_ENVS) * first_reset
    rows_c = np.concatenate([obs0_c[None], clean['obs'][:-1]], 0)
    # a left-out (step, env) is stood in for by the clean run's rows and actions: a valid pair under the same (seed, step, row) key
    rows_in, act_in = np.where(want[:, :, None, None], rows_c, rows), np.where(want[:, :, None], clean['act'], out['act'])
    assert np.isfinite(rows_in[1:]).all() and np.array_equal(rows_in[:, others], rows[:, others])
    assert_rollout_actions_match_f64(net, 9, 0, rows_in, act_in, 'non-finite %s' % name)


# ---- the learner -------------------------------------------------------------------------------------------------------------------
def _poisoned_memory(ug):
    _, _, _, ring_kw, N, D = ug.VARIANTS['attention']
    rb = ug._filled_memory(ring_kw, N, D)
    rb.obs[::8, 1, 3] = nf.NAN                                      # one obs element of every eighth slot
    return rb


@pytest.mark.parametrize('switches', ['none', 'all', 'all-graphed'])
def test_one_update_on_a_poisoned_batch_gives_nan_losses(switches):
    """A NaN observation row in the batch: the unfused learner's losses are NaN -- a visible failure, and what the reference does.  With
    every switch (fused front, LSTM, attention, sampling, optimizer, targets), eager and graphed, the same update must say so too."""
    import tests.test_gpu_update_graph as ug                        # the harness: VARIANTS, _filled_memory, BATCH; examples/ on sys.path
    import madr_learner
    from multiagent_rl_amd import critic as cr, dense, policy as pol
    rb = _poisoned_memory(ug)
    first = rb.make_index(ug.BATCH)                                 # the first batch of every learner below: the draw is keyed
    rb.reset_draws(0)
    assert bool((first % 8 == 0).any()) and bool(torch.isnan(rb.obs[first]).any())
    torch.manual_seed(3)
    _, mk_actor, mk_critic, _, _, _ = ug.VARIANTS['attention']
    kw = {} if switches == 'none' else dict(fused_optimizer=True, fused_lstm=True, fused_attention=True, fused_sampling=True,
                                            sampling_seed=5, fused_front=True, graph_update=switches == 'all-graphed')
    t = madr_learner.Trainer(mk_actor(pol, cr), mk_critic(pol, cr), rb, batch_size=ug.BATCH, **kw)
    if switches == 'all':
        pol.accelerate_trainer(t, targets=True)
    assert isinstance(t.critic, dense.FusedFront) == (switches != 'none')
    torch.manual_seed(100)
    loss_actor, loss_critic = (float(x) for x in t.optimize())    # the graphed update returns device tensors
    print('%s: losses %r %r' % (switches, loss_actor, loss_critic))
    assert loss_actor != loss_actor and loss_critic != loss_critic, (switches, loss_actor, loss_critic)
