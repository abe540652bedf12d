"""CPU: the reference ledger of the episode statistics (tests/episode_ledger_ref.py) and the inputs the GPU tests feed the nine HIP
producers with (tests/test_gpu_episode_stats.py).  The ledger is checked against a plain per-env loop; every input generator against
the conditions it promises; and two sharpness checks show that the GPU assertions CAN fail: a float32 accumulator breaks the
finished_sum bound, a terminal flag on the neighbouring env changes episode_return."""
import math

import numpy as np
import pytest

from tests import episode_ledger_ref as el

# the (B, T) of every synthetic GPU case: producers 1 and 2 are single-step, producer 3 walks T steps
STATS_B = (1, 63, 1023, 1024, 1025, 3000)
TAIL_B = (1, 255, 256, 257, 1023, 1025, 2500)
ROLLOUT_BT = ((1, 1), (255, 7), (256, 8), (257, 9), (600, 17), (300, 31))
ALL_BT = sorted(set([(b, 1) for b in STATS_B + TAIL_B] + list(ROLLOUT_BT)))


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


@pytest.mark.parametrize('B,T', [(1, 1), (1, 5), (7, 1), (33, 9), (257, 17)])
def test_vectorised_ledger_equals_the_per_env_loop(B, T):
    case = el.synthetic_case(B, T, calls=1, seed=3)
    a = el.ledger(case['rew'][0], case['terminal'][0], case['ret0'], case['sum0'], case['count0'])
    b = el.ledger_loop(case['rew'][0], case['terminal'][0], case['ret0'], case['sum0'], case['count0'])
    assert np.array_equal(_bits(a['episode_return']), _bits(b['episode_return']))
    for k in ('finished_count', 'finished_sum', 'abs_sum', 'n'):
        assert a[k] == b[k], k
    assert a['n'] == 1 + int(case['terminal'][0].sum()) and a['finished_count'] == case['count0'] + a['n'] - 1


def test_ledger_on_a_hand_computed_example():
    rew = np.array([[1.0, -2.0], [0.5, 4.0], [0.25, 8.0]], np.float32)
    term = np.array([[False, True], [False, False], [True, True]])
    w = el.ledger(rew, term, np.array([10.0, 100.0], np.float32), 1000.0, 5)
    assert w['finished'].tolist() == [98.0, 11.75, 12.0]            # (step, env) order; the carry-ins 100 and 10 are inside
    assert w['episode_return'].tolist() == [0.0, 0.0] and w['finished_count'] == 8
    assert w['finished_sum'] == 1121.75 and w['abs_sum'] == 1121.75 and w['n'] == 4
    assert el.bound(4, 1.0) == 4 * 2.0 ** -53 / (1 - 4 * 2.0 ** -53)
    nothing = el.ledger(rew[:2], np.zeros((2, 2), bool), np.zeros(2, np.float32), 0.0, 0)
    assert nothing['finished_count'] == 0 and nothing['n'] == 1 and nothing['episode_return'].tolist() == [1.5, 2.0]


def test_running_return_is_rounded_to_float32_every_step():
    """1e4 + 1e-3 is not a float32: the ledger must round where the kernels round."""
    rew = np.array([[1e4], [1e-3], [1e-3]], np.float32)
    w = el.ledger(rew, np.array([[False], [False], [True]]), np.zeros(1, np.float32), 0.0, 0)
    want = np.float32(np.float32(np.float32(1e4) + np.float32(1e-3)) + np.float32(1e-3))
    assert w['finished'][0] == want and float(want) != 1e4 + 2e-3


@pytest.mark.parametrize('B,T', ALL_BT)
def test_synthetic_inputs_fulfil_their_conditions(B, T):
    case = el.synthetic_case(B, T, calls=2, seed=11)
    assert case['rew'].shape == (2, T, B) and case['rew'].dtype == np.float32 and case['terminal'].dtype == bool
    el.assert_case_conditions(case)
    again = el.synthetic_case(B, T, calls=2, seed=11)
    assert all(np.array_equal(case[k], again[k]) for k in ('rew', 'terminal', 'ret0'))


@pytest.mark.parametrize('B,T,L', [(37, 20, 7), (5, 20, 7), (17, 12, 7), (48, 20, 7), (3200, 8, 3)])
def test_desynchronised_clocks_end_episodes_on_different_steps(B, T, L):
    """The rollout cases start from ep_step = arange(B) % max_episode_len: the ends are spread over the steps, every env ends two or
    three times in a launch (once or twice in the shortened wide-row case), and a second launch continues the clocks."""
    ep0 = np.arange(B) % L
    term = el.clock_terminals(ep0, T, L)
    per_env = term.sum(0)
    assert per_env.min() >= T // L and per_env.max() <= T // L + 1 and per_env.max() >= 2
    if B >= L:
        assert term.any(1).all() and not term.all(1).any()          # some env ends on every step, never all of them
        assert len(set(per_env.tolist())) == (2 if T % L else 1)
    cont = el.clock_terminals((ep0 + T) % L, T, L)
    assert np.array_equal(np.concatenate([term, cont]), el.clock_terminals(ep0, 2 * T, L))
    # what the clock formula restates: a counter that ends the episode when it reaches L
    c, want = ep0.copy(), np.zeros((T, B), bool)
    for t in range(T):
        c = c + 1
        want[t] = c >= L
        c[want[t]] = 0
    assert np.array_equal(term, want)


@pytest.mark.parametrize('B,T', [(3000, 1), (600, 17), (300, 31)])
def test_a_float32_accumulator_violates_the_bound(B, T):
    """Sharpness of the finished_sum tolerance: summing the finished returns in float32, in index order, misses the ledger by far more
    than gamma_n * abs_sum on the mixed-magnitude input -- a kernel that accumulated in float32 would fail the GPU test.  A float64
    accumulation in index order, in reverse order and as a pairwise tree all stay inside."""
    case = el.synthetic_case(B, T, calls=1, seed=11)
    w = el.ledger(case['rew'][0], case['terminal'][0], case['ret0'], case['sum0'], case['count0'])
    tol = el.bound(w['n'], w['abs_sum'])
    acc32 = np.float32(0.0)
    for r in w['finished']:
        acc32 = np.float32(acc32 + r)
    got32 = case['sum0'] + float(acc32)
    assert abs(got32 - w['finished_sum']) > 1e3 * tol, (abs(got32 - w['finished_sum']), tol)
    terms = [case['sum0']] + [float(r) for r in w['finished']]
    fwd = 0.0
    for x in terms:
        fwd += x
    rev = 0.0
    for x in reversed(terms):
        rev += x
    tree = list(terms)
    while len(tree) > 1:
        tree = [tree[i] + tree[i + 1] if i + 1 < len(tree) else tree[i] for i in range(0, len(tree), 2)]
    for got in (fwd, rev, tree[0]):
        assert abs(got - w['finished_sum']) <= tol
    assert tol < 1e-9 * abs(w['finished_sum'])                      # and it asks more than the kernel-against-kernel tests' 1e-9


@pytest.mark.parametrize('B,T', [(63, 1), (257, 9), (300, 31)])
def test_a_terminal_flag_on_the_neighbouring_env_changes_episode_return(B, T):
    """Sharpness of the bit-equality of episode_return: move ONE terminal flag to the env next door and the ledger's running returns
    differ at both envs -- a kernel that cleared the wrong env's return would fail the GPU test."""
    case = el.synthetic_case(B, T, calls=1, seed=11)
    rew, term = case['rew'][0], case['terminal'][0]
    w = el.ledger(rew, term, case['ret0'], case['sum0'], case['count0'])
    t = T - 1
    e = next(e for e in range(B - 1) if term[t, e] and not term[t, e + 1])
    shifted = term.copy()
    shifted[t, e], shifted[t, e + 1] = False, True
    s = el.ledger(rew, shifted, case['ret0'], case['sum0'], case['count0'])
    differs = np.flatnonzero(_bits(w['episode_return']) != _bits(s['episode_return']))
    assert differs.tolist() == [e, e + 1]
    assert s['finished_count'] == w['finished_count']               # the count alone would not notice
    assert abs(s['finished_sum'] - w['finished_sum']) > el.bound(w['n'], w['abs_sum'])


def test_check_accepts_the_ledger_and_refuses_each_kind_of_error():
    case = el.synthetic_case(257, 9, calls=1, seed=11)
    w = el.ledger(case['rew'][0], case['terminal'][0], case['ret0'], case['sum0'], case['count0'])
    el.check(w['episode_return'], w['finished_sum'], w['finished_count'], w)
    bad = w['episode_return'].copy()
    bad[5] = np.nextafter(bad[5], np.float32(np.inf)) if bad[5] != 0 else np.float32(1e-30)
    with pytest.raises(AssertionError, match='episode_return'):
        el.check(bad, w['finished_sum'], w['finished_count'], w)
    with pytest.raises(AssertionError, match='finished_count'):
        el.check(w['episode_return'], w['finished_sum'], w['finished_count'] + 1, w)
    with pytest.raises(AssertionError, match='finished_sum'):
        el.check(w['episode_return'], w['finished_sum'] * (1 + 1e-9), w['finished_count'], w)
    assert math.isfinite(el.bound(w['n'], w['abs_sum']))
