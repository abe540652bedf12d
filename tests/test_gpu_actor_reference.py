"""GPU: every actor kernel instance against the float64 host reference (oracle/actor_oracle.py).

(a) The hidden state H = relu(BiLSTM(relu(dense1(x)))) and the logits of pw_actor_fused16_kernel<S1C> and
    pw_actor_fused_kernel<S1C> (S1C = 1 .. 8, each at two or more N), of the three-launch chain (PW_ACTOR_NO_FUSE, and N > 96)
    and of its PW_ACTOR_NO_MFMA form, within 2e-5 of the float64 forward, on random rows, on the C oracle's observation rows
    and on rows that saturate the gates (SAT_ATOL).
(b) The sampled actions equal the host's restatement of the Gumbel draw (Philox keyed by seed, step and global row, the
    uniform formed in float32 as the device forms it, log(-log u) in float64) at every (row, head) whose float64 margin
    exceeds 1e-4 -- a logit error of 2e-5 plus the float32 rounding of the noise stays far below it.
(c) A logit that draws the top Philox word (w >> 8 == 2^24 - 1) and carries a -50 bias is not chosen (before the uniform
    was clamped below 1 that word gave u == 1.0, noise -inf, and the logit won whatever its value).

``PW_ACTOR_F64_REPORT=<path>``: the measured worst |dH|, |dlogit| and the undecided share per case are appended there
(profiles/actor_vs_f64.txt holds such a run).
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

from oracle import actor_oracle as ao  # noqa: E402  (checker only)
from oracle import c_oracle as co  # noqa: E402

ATOL = 2e-5          # the bar of the float32 PyTorch comparisons (tests/test_gpu_engine.py)
SAT_ATOL = 2e-5      # saturated gates (inputs x 30, |c| up to N): worst measured |dH| 5.1e-06, |dlogit| 1.2e-05 (profiles/actor_vs_f64.txt),
                     # so the saturation case is held to the same bar
MARGIN = 1e-4        # (row, head) pairs whose float64 margin is at or below this are not asserted (counted instead)

HEADS = [(5,), (5, 10), (7, 9), (1, 15), (16,), (1,)]
N16 = [1, 2, 3, 6, 7, 12, 13, 16]                           # pw_actor_fused16_kernel
NF = [17, 24, 30, 31, 32, 33, 48, 50, 64, 95, 96]           # pw_actor_fused_kernel
D_OF_S1C = {1: (1, 8), 2: (9, 16), 3: (21, 24), 4: (32, 25), 5: (33, 40), 6: (44, 48), 7: (52, 56), 8: (57, 64)}
# (seed, call index, head shift): call 2^32 + 3 exercises the step's high word, seeds >= 2^32 the key's; b2 -= 30 makes every
# real logit negative (a padded word past OUT would win if it competed), 'const' zeroes the head (the noise alone decides)
VARIANTS = [(9, 0, 0.0), (2 ** 32 + 77, 1, -30.0), (123, 2 ** 32 + 3, 30.0), (5, 1, 'const'), (2 ** 33 + 1, 0, 0.0),
            (31, 2 ** 32 + 3, -30.0)]

def _report(line):
    path = os.environ.get('PW_ACTOR_F64_REPORT')
    if path:
        with open(path, 'a') as f:
            f.write(line + '\n')


def _kernel_cases():
    """(kernel, S1C, N, D, heads, variant): every S1C at two N per kernel, every N at least once."""
    out = []
    for kern, ns, off in (('fused16', N16, 3), ('fused', NF, 4)):
        for i, s1c in enumerate(range(1, 9)):
            for j in range(2):
                k = 2 * i + j + (0 if kern == 'fused16' else 1)
                out.append((kern, s1c, ns[(i + j * off) % len(ns)], D_OF_S1C[s1c][j], HEADS[k % 6], k % 6))
    return out


def _ragged_batch(N, kern, rows=600):
    E = 16 if kern == 'fused16' else min(16, 96 // N)
    return E * max(1, rows // (E * N)) + 1                   # the last workgroup holds one environment


def _make_net(D, heads, shift, seed):
    from multiagent_rl_amd.policy import ActorNetwork
    torch.manual_seed(seed)
    net = ActorNetwork(D, list(heads) if len(heads) == 2 else heads[0]).eval()
    hs = [net.dense2_1.module, net.dense2_2.module] if len(heads) == 2 else [net.dense2.module]
    with torch.no_grad():
        for h in hs:
            if shift == 'const':
                h.weight.zero_()
                h.bias.zero_()
            else:
                h.bias += shift
    return net.cuda()


def _device_kernel(fused, N):
    """The kernel pw_actor_fused / the chain actually runs (pworld_policy.hip: N <= 16 goes to the 16-wide kernel when
    actor16_lds_floats(N, 16 N, 4 S1C) fits 160 KiB, which holds for every D <= 64)."""
    if not fused.use_fused or N > 96:
        return 'chain' if fused.use_mfma_front else 'chain-nomfma'
    S1 = 4 * ((fused.w1.shape[1] + 7) // 8)
    lds16 = (N * 1024 + 2048 + N * 1024 + 2 * S1 * 64 + 64) * 4
    return 'fused16' if N <= 16 and lds16 <= 160 * 1024 else 'fused'


def run_and_compare(fused, net, obs, seed, calls, label, atol=ATOL, check_act=True, atol_logit=None):
    """obs float32 numpy [B, N, D] -> dict of measured errors; asserts H within ``atol`` and the logits within ``atol_logit``
    (default ``atol``) of the float64 forward, and the actions equal ao.predict at margin > MARGIN."""
    atol_logit = atol if atol_logit is None else atol_logit
    heads = fused.heads
    B, N, _ = obs.shape
    x = torch.from_numpy(obs).cuda()
    H = fused.hidden(x).cpu().numpy()
    lg = fused.logits(x)
    lg = (torch.cat(lg, -1) if isinstance(lg, list) else lg).cpu().numpy()
    fused.calls = calls
    act = fused(x).cpu().numpy().reshape(B * N, len(heads))
    H64, lg64 = ao.forward_f64(net, obs)
    lg64 = np.concatenate(lg64, -1)
    assert np.isfinite(H).all() and np.isfinite(lg).all(), label
    dH, dL = float(np.abs(H - H64).max()), float(np.abs(lg - lg64).max())
    res = dict(dH=dH, dL=dL, undecided=0, pairs=B * N * len(heads))
    assert dH <= atol and dL <= atol_logit, '%s: |dH| %.3g |dlogit| %.3g (bounds %.3g, %.3g)' % (label, dH, dL, atol, atol_logit)
    if check_act:
        want, margin = ao.predict(lg64.reshape(B * N, -1), seed, calls, np.arange(B * N), heads)
        ok = margin > MARGIN
        bad = np.argwhere(ok & (act != want))
        assert bad.size == 0, '%s: %d actions differ from the float64 prediction, first (row, head) %s: got %d want %d margin %.3g' % (
            label, len(bad), tuple(bad[0]), act[tuple(bad[0])], want[tuple(bad[0])], margin[tuple(bad[0])])
        res['undecided'] = int((~ok).sum())
        assert res['undecided'] <= max(1, 1e-3 * res['pairs']), '%s: %d of %d (row, head) pairs undecided' % (
            label, res['undecided'], res['pairs'])
    _report('%-58s |dH| %.2e  |dlogit| %.2e  undecided %d / %d' % (label, dH, dL, res['undecided'], res['pairs']))
    return res


@pytest.mark.parametrize('kern,S1C,N,D,heads,var', _kernel_cases(),
                         ids=['%s-S1C%d-N%d-D%d-h%s' % (c[0], c[1], c[2], c[3], 'x'.join(map(str, c[4]))) for c in _kernel_cases()])
def test_one_launch_actor_matches_float64(kern, S1C, N, D, heads, var):
    from multiagent_rl_amd.policy import FusedActor
    assert (D + 7) // 8 == S1C
    seed, calls, shift = VARIANTS[var]
    net = _make_net(D, heads, shift, seed=N * 100 + D)
    fused = FusedActor(net, seed=seed)
    assert _device_kernel(fused, N) == kern
    B = _ragged_batch(N, kern)
    rng = np.random.RandomState(N + D)
    label = '%s<S1C=%d> N=%d D=%d B=%d heads=%s seed=%d call=%d shift=%s' % (kern, S1C, N, D, B, heads, seed, calls, shift)
    run_and_compare(fused, net, (rng.randn(B, N, D) * 2).astype(np.float32), seed, calls, label)
    sat = (rng.randn(B, N, D) * 30).astype(np.float32)
    run_and_compare(fused, net, sat, seed, calls, label + ' saturated', atol=SAT_ATOL, check_act=False)


@pytest.mark.parametrize('mode', ['nofuse', 'nomfma'])
@pytest.mark.parametrize('N,D,var', [(1, 8, 0), (6, 16, 1), (13, 21, 2), (31, 33, 3), (96, 64, 4), (100, 9, 5)])
def test_three_launch_chain_matches_float64(monkeypatch, mode, N, D, var):
    from multiagent_rl_amd.policy import FusedActor
    seed, calls, shift = VARIANTS[var]
    net = _make_net(D, (5,), shift, seed=N + D)
    monkeypatch.setenv('PW_ACTOR_NO_FUSE', '1')
    if mode == 'nomfma':
        monkeypatch.setenv('PW_ACTOR_NO_MFMA', '1')
    fused = FusedActor(net, seed=seed)
    assert _device_kernel(fused, N) == ('chain' if mode == 'nofuse' else 'chain-nomfma')
    B = 16 * max(1, 600 // (16 * N)) + 1
    rng = np.random.RandomState(N * D)
    label = '%s N=%d D=%d B=%d seed=%d call=%d shift=%s' % (_device_kernel(fused, N), N, D, B, seed, calls, shift)
    run_and_compare(fused, net, (rng.randn(B, N, D) * 2).astype(np.float32), seed, calls, label)
    run_and_compare(fused, net, (rng.randn(B, N, D) * 30).astype(np.float32), seed, calls, label + ' saturated',
                    atol=SAT_ATOL, check_act=False)


def test_chain_beyond_96_agents_is_the_default_route():
    from multiagent_rl_amd.policy import FusedActor
    net = _make_net(16, (5,), 0.0, seed=3)
    fused = FusedActor(net, seed=2 ** 32 + 9)
    assert fused.use_fused and _device_kernel(fused, 100) == 'chain'
    obs = (np.random.RandomState(1).randn(7, 100, 16) * 2).astype(np.float32)
    run_and_compare(fused, net, obs, fused.seed, 2 ** 32 + 3, 'chain (default route) N=100 D=16 B=7')


@pytest.mark.parametrize('N,D,heads', [(1, 8, (5,)), (6, 16, (5, 10)), (13, 33, (7, 9)), (16, 64, (1, 15))])
def test_bf16x3_actor_matches_float64(N, D, heads):
    """The opt-in bf16x3 input projection (N <= 16): held to the same 2e-5 and to the same sampled actions."""
    from multiagent_rl_amd import _lib
    from multiagent_rl_amd.policy import FusedActor
    lib = _lib.load()
    net = _make_net(D, heads, 0.0, seed=N)
    fused = FusedActor(net, seed=2 ** 32 + N)
    B = 16 * max(1, 600 // (16 * N)) + 1
    obs = (np.random.RandomState(D).randn(B, N, D) * 2).astype(np.float32)
    prev = lib.pw_actor_set_bf16x3(1)
    try:
        run_and_compare(fused, net, obs, fused.seed, 2 ** 32 + 3, 'fused16 bf16x3 N=%d D=%d B=%d heads=%s' % (N, D, B, heads))
    finally:
        lib.pw_actor_set_bf16x3(prev)


def _oracle_rows(scenario, B, N=None, adv=None):
    if scenario == 'simple_reference':
        cfg = co.make_config(scenario, seed=17)
        o = co.CRefOracle(cfg, B, np.float32)
    elif scenario == 'simple_tag':
        cfg = co.make_config(scenario, N, num_adversaries=adv, seed=31)
        o = co.COracle(cfg, B, np.float32)
    else:
        cfg = co.make_config(scenario, N, seed=21)
        o = co.COracle(cfg, B, np.float32)
    rows = [o.reset()]
    rng = np.random.RandomState(0)
    for _ in range(3):      # rows with velocities and (simple_reference) communication in them
        n = o.N
        w = o.step(act_idx=rng.randint(0, 5, (B, n)), act_comm=rng.randint(0, 10, (B, n))) if scenario == 'simple_reference' \
            else o.step(act_idx=rng.randint(0, 5, (B, n)))
        rows.append(w['obs'])
    return np.ascontiguousarray(np.concatenate(rows, 0), np.float32)


@pytest.mark.parametrize('scenario,N,adv,heads', [('simple_spread', 3, None, (5,)), ('simple_spread', 6, None, (5,)),
                                                  ('simple_spread', 12, None, (5,)), ('simple_spread', 24, None, (5,)),
                                                  ('simple_spread', 30, None, (5,)), ('simple_tag', 6, 4, (5,)),
                                                  ('simple_reference', 2, None, (5, 10))])
def test_actor_on_oracle_observation_rows_matches_float64(scenario, N, adv, heads):
    """Real observation rows (simple_tag: the good agents' rows zero-padded as the env returns them)."""
    from multiagent_rl_amd.policy import FusedActor
    obs = _oracle_rows(scenario, 65, N, adv)
    D = obs.shape[2]
    net = _make_net(D, heads, 0.0, seed=N)
    fused = FusedActor(net, seed=2 ** 32 + 1)
    kern = _device_kernel(fused, obs.shape[1])
    run_and_compare(fused, net, obs, fused.seed, 7, '%s %s N=%d D=%d B=%d oracle rows' % (kern, scenario, N, D, obs.shape[0]))


@pytest.mark.parametrize('mode,N', [('fused16', 6), ('fused', 24), ('chain', 6)])
def test_top_philox_word_does_not_force_its_logit(monkeypatch, mode, N):
    """Row 5 at step 0 draws the top word for logit q; q carries a -50 bias.  The action must be the host's prediction (not q)
    and nothing may be NaN."""
    from multiagent_rl_amd.policy import FusedActor
    seed, q = ao.find_top_word_seed(5, 0, start=2 ** 32)
    D = 16
    net = _make_net(D, (5,), 0.0, seed=1)
    with torch.no_grad():
        net.dense2.module.bias[q] -= 50.0
    if mode == 'chain':
        monkeypatch.setenv('PW_ACTOR_NO_FUSE', '1')
    fused = FusedActor(net, seed=seed)
    assert _device_kernel(fused, N) == mode
    obs = (np.random.RandomState(2).randn(33, N, D) * 2).astype(np.float32)
    assert int(ao.gumbel_words(seed, 0, [5], 5)[0, q]) >> 8 == ao.TOP_WORD
    # logit q sits near -50: its 64 float32 accumulations round at ulp(50) / 2 each (measured 2.4e-5 on all three forms)
    run_and_compare(fused, net, obs, seed, 0, '%s N=%d top word at (row 5, logit %d)' % (mode, N, q),
                    atol_logit=ATOL + 64 * 2.0 ** -24 * 50)
    fused.calls = 0
    act = fused(torch.from_numpy(obs).cuda()).cpu().numpy().reshape(-1)
    want, _ = ao.predict(ao.forward_f64(net, obs)[1][0].reshape(-1, 5), seed, 0, np.arange(33 * N), (5,))
    assert act[5] != q and act[5] == want[5, 0]


# ------------------------------------------------------------------ one-launch rollouts (used by test_gpu_policy_oracle.py)
def assert_rollout_actions_match_f64(net, seed, step0, rows_seen, act, label, max_rows=400000):
    """rows_seen [T, B, N, D]: the observation rows the policy saw at steps step0 .. step0 + T - 1 (the reset rows, then the
    post-reset rows of each step); act [T, B, N] or [T, B, N, 2]: what the launch sampled.  Asserts equality with the host
    prediction at margin > MARGIN.  Steps are subsampled (every k-th, the first and last kept) when T B N exceeds
    ``max_rows``.  -> (pairs checked, undecided)."""
    rows_seen = np.asarray(rows_seen, np.float32)
    T, B, N, _ = rows_seen.shape
    heads = tuple(net.out_dim) if type(net.out_dim) is list else (net.out_dim,)
    act = np.asarray(act).reshape(T, B * N, len(heads))
    k = max(1, -(-T * B * N // max_rows))
    steps = sorted(set(range(0, T, k)) | {T - 1})
    P = ao.actor_params(net)
    pairs = undecided = 0
    for t in steps:
        lg = np.concatenate(ao.forward_f64(P, rows_seen[t])[1], -1).reshape(B * N, -1)
        want, margin = ao.predict(lg, seed, step0 + t, np.arange(B * N), heads)
        ok = margin > MARGIN
        bad = np.argwhere(ok & (act[t] != want))
        assert bad.size == 0, '%s step %d: %d actions differ from the float64 prediction, first (row, head) %s: got %d want %d' % (
            label, t, len(bad), tuple(bad[0]), act[t][tuple(bad[0])], want[tuple(bad[0])])
        pairs += ok.size
        undecided += int((~ok).sum())
    assert undecided <= max(1, 1e-3 * pairs), '%s: %d of %d undecided' % (label, undecided, pairs)
    _report('%-58s steps %d of %d  undecided %d / %d' % (label, len(steps), T, undecided, pairs))
    return pairs, undecided


def test_spread_rollout_top_word_at_the_first_step():
    """The one-launch simple_spread rollout (default form, N = 6): the top word at (row 5, step 0) does not force its logit."""
    from multiagent_rl_amd import make_batched_env
    from multiagent_rl_amd.policy import FusedActor
    seed, q = ao.find_top_word_seed(5, 0, start=2 ** 32)
    B, N, T = 33, 6, 3
    env = make_batched_env('simple_spread', B, n=N, auto_reset=True, max_episode_len=25, seed=21)
    cfg = co.make_config('simple_spread', N, max_episode_len=25, auto_reset=True, seed=21)
    o32 = co.COracle(cfg, B, np.float32)
    net = _make_net(env.obs_dim, (5,), 0.0, seed=4)
    with torch.no_grad():
        net.dense2.module.bias[q] -= 50.0
    fused = FusedActor(net, seed=seed)
    obs0 = o32.reset()
    assert np.array_equal(env.reset().cpu().numpy(), obs0)
    got = fused.rollout(env, T)
    a = got['act'].cpu().numpy()
    assert np.isfinite(got['obs'].cpu().numpy()).all()
    rows = np.concatenate([obs0[None], got['obs'][:-1].cpu().numpy()], 0)
    assert_rollout_actions_match_f64(fused.actor, seed, 0, rows, a, 'spread rollout N=6 top word (row 5, logit %d)' % q)
    assert a[0].reshape(-1)[5] != q
