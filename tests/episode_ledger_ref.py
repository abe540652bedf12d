"""Reference ledger of the rollout's episode statistics (experiments/run.py:55-65), numpy only.

run.py keeps one running return per env: ``episode_return += shared reward`` every step; where the step ended the episode the return
goes onto the list of finished returns and is cleared.  ``mean_episode_reward`` = sum of that list / its length.  Every HIP producer of
these numbers (pw_episode_stats, pw_replay_add_tail, pw_replay_add_rollout, the statistics sink of the one-launch rollouts) keeps the
running return in float32, in step order, and adds the finished returns up in float64 in an order of its own.  The ledger restates that
with the one summation no order can beat: ``math.fsum`` (exact, rounded once).

Tolerance for ``finished_sum`` (derived, not measured): a producer adds the same n float64 terms -- the carry-in ``sum0`` and every
finished return -- in some fixed order, each addition rounding once (u = 2**-53).  For ANY order or tree of those additions
|got - exact| <= gamma_(n-1) * sum|term| (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2), and fsum is within half
an ulp of exact; ``bound()`` returns gamma_n * abs_sum, n = number of terms, which covers both.  ``episode_return`` and ``finished_count``
have no tolerance.
"""
import math

import numpy as np

U = 2.0 ** -53


def bound(n, abs_sum):
    """gamma_n * abs_sum, gamma_n = n u / (1 - n u)."""
    return n * U / (1.0 - n * U) * abs_sum


def ledger(rew_shared, terminal, ret0, sum0, count0):
    """rew_shared [T,B] float32, terminal [T,B] bool, ret0 [B] float32 (running returns carried in), sum0 float64, count0 int ->
    dict(episode_return [B] float32 (expected bit for bit), finished_count (exact int), finished_sum (fsum over sum0 and every finished
    return widened to float64), abs_sum = |sum0| + sum |r_i|, n = number of terms, finished = the finished returns in (step, env) order
    as float32)."""
    rew = np.asarray(rew_shared)
    term = np.asarray(terminal).astype(bool)
    assert rew.dtype == np.float32 and rew.ndim == 2 and term.shape == rew.shape
    ret = np.array(ret0, dtype=np.float32, copy=True)
    assert ret.shape == (rew.shape[1],)
    finished = []
    for t in range(rew.shape[0]):
        ret = ret + rew[t]                      # float32 + float32 -> float32, one rounding, as `ret + rw` in the kernels
        assert ret.dtype == np.float32
        finished.append(ret[term[t]].copy())    # env order within the step
        ret[term[t]] = np.float32(0.0)
    finished = np.concatenate(finished) if finished else np.zeros(0, np.float32)
    terms = [float(sum0)] + [float(r) for r in finished.astype(np.float64)]
    return dict(episode_return=ret, finished_count=int(count0) + int(finished.size), finished_sum=math.fsum(terms),
                abs_sum=math.fsum(abs(x) for x in terms), n=len(terms), finished=finished)


def ledger_loop(rew_shared, terminal, ret0, sum0, count0):
    """The same, written as run.py writes it: one env at a time, one step at a time, Python lists.  (The finished returns come out in
    (env, step) order here; fsum does not care.)"""
    T, B = np.asarray(rew_shared).shape
    out_ret = np.zeros(B, np.float32)
    done = []
    for e in range(B):
        r = np.float32(ret0[e])
        for t in range(T):
            r = np.float32(r + np.float32(rew_shared[t][e]))
            if terminal[t][e]:
                done.append(float(r))
                r = np.float32(0.0)
        out_ret[e] = r
    terms = [float(sum0)] + done
    return dict(episode_return=out_ret, finished_count=int(count0) + len(done), finished_sum=math.fsum(terms),
                abs_sum=math.fsum(abs(x) for x in terms), n=len(terms))


def check(got_return, got_sum, got_count, want, label=''):
    """The three assertions every producer must pass against ``want = ledger(...)``; prints the figures first."""
    err, tol = abs(float(got_sum) - want['finished_sum']), bound(want['n'], want['abs_sum'])
    print('%s: finished_count %d (ledger %d), finished_sum %.17g (ledger %.17g), |diff| %.3g, bound %.3g over %d terms'
          % (label, int(got_count), want['finished_count'], float(got_sum), want['finished_sum'], err, tol, want['n']))
    got_return = np.asarray(got_return)
    assert got_return.dtype == np.float32
    assert np.array_equal(got_return.view(np.uint32), want['episode_return'].view(np.uint32)), \
        '%s: episode_return differs from the ledger at envs %s' % (
            label, np.flatnonzero(got_return.view(np.uint32) != want['episode_return'].view(np.uint32))[:8])
    assert int(got_count) == want['finished_count'], '%s: finished_count %d, ledger %d' % (label, int(got_count), want['finished_count'])
    assert err <= tol, '%s: finished_sum %.17g, ledger %.17g: off by %.3g > gamma_n * abs_sum = %.3g' % (
        label, float(got_sum), want['finished_sum'], err, tol)


# ------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------
def synthetic_case(B, T, calls=2, seed=0):
    """Inputs for ``calls`` consecutive launches of one producer into the same accumulators: dict(rew [calls,T,B] float32,
    terminal [calls,T,B] bool, ret0 [B] float32, sum0 float, count0 int).  What it guarantees (``assert_case_conditions`` checks it on
    the ledger alone):
      - some env finishes no episode in some call (B >= 2: in every call; B = 1: the last call has no terminal at all);
      - T >= 2: some env finishes two episodes inside one call, the second of them on the call's LAST step (the clamped tail of an 8-deep
        walk), the first on its first step;
      - every carry-in return is non-zero, and one of them lands in an episode that finishes on the first step of the first call;
      - the three accumulators start non-zero;
      - rewards of both signs with magnitudes from 1e-3 to 1e4 (log-uniform; the two extremes are always present);
      - the ends are desynchronised: everywhere else a terminal flag is an independent coin."""
    rng = np.random.RandomState(1000003 * seed + 7919 * B + T)
    n = calls * T * B
    expo = rng.uniform(-3.0, 4.0, n)
    sign = np.where(rng.rand(n) < 0.5, -1.0, 1.0)
    expo[0], sign[0] = -3.0, 1.0
    expo[-1], sign[-1] = 4.0, -1.0
    rew = (sign * 10.0 ** expo).astype(np.float32).reshape(calls, T, B)
    term = rng.rand(calls, T, B) < min(0.4, 2.5 / T)
    for c in range(calls):
        if B >= 2:
            quiet, busy = (B - 1, 0) if c % 2 == 0 else (0, B - 1)
            term[c, :, quiet] = False
        else:
            busy = 0
            if c == calls - 1:
                term[c] = False
                continue
        term[c, 0, busy] = True
        term[c, T - 1, busy] = True
    ret0 = (np.where(rng.rand(B) < 0.5, -1.0, 1.0) * 10.0 ** rng.uniform(-2.0, 3.0, B)).astype(np.float32)
    return dict(rew=rew, terminal=term, ret0=ret0, sum0=-12345.678, count0=41)


def assert_case_conditions(case):
    """The guarantees of ``synthetic_case``, asserted on the reference alone."""
    rew, term, ret0 = case['rew'], case['terminal'], case['ret0']
    calls, T, B = rew.shape
    per_env = term.sum(1)                                     # [calls, B] episodes finished per call and env
    assert (per_env == 0).any(), 'no env without a finished episode'
    if B >= 2:
        assert (per_env == 0).any(1).all() and (per_env > 0).any(1).all()
    if T >= 2:
        assert (per_env >= 2).any(), 'no env finishes two episodes inside one call'
        assert ((per_env >= 2) & term[:, T - 1, :]).any(), 'no second episode ends on the last step'
    assert (ret0 != 0).all() and term[0, 0].any()
    first = ledger(rew[0, :1], term[0, :1], ret0, 0.0, 0)     # the carry-in is part of a finished return
    no_carry = ledger(rew[0, :1], term[0, :1], np.zeros_like(ret0), 0.0, 0)
    assert first['finished'].size > 0 and not np.array_equal(first['finished'], no_carry['finished'])
    assert case['sum0'] != 0 and case['count0'] != 0
    a = np.abs(rew.astype(np.float64))
    assert (rew > 0).any() and (rew < 0).any()
    assert a.min() >= 0.999e-3 and a.min() <= 1.001e-3 and a.max() <= 1.001e4 and a.max() >= 0.999e4
    if B >= 8 and T == 1:
        assert len(set(per_env[0].tolist())) > 1              # not every env ends at once


def clock_terminals(ep_step0, T, max_episode_len):
    """terminal [T,B] of an auto-resetting env whose episode clocks start at ``ep_step0`` [B]: the step that takes the clock to
    ``max_episode_len`` ends the episode (run.py:50) and the reset puts it back to 0."""
    e = np.asarray(ep_step0, dtype=np.int64)[None, :] + np.arange(T, dtype=np.int64)[:, None]
    return (e % max_episode_len) == max_episode_len - 1
