"""Reference model of the episode log (pw_episode_log_absorb, train.EpisodeLog), numpy and plain Python only.

The contract, restated as the loop experiments/run.py:55-65 writes, for B worlds stepped side by side:

  sums   one env at a time, one step at a time, Python floats (IEEE double; a float32 reward widens exactly):
             for i, rew in enumerate(rew_n): total += rew; by_agent[i] += rew            (run.py:55-57)
         so ``total`` is a sum of its own over the agents in ascending order, not the sum of the shares.  Where the step ends the
         episode the sums are stored and the running sums become +0.0 BY ASSIGNMENT (a NaN or Inf poisons its own episode only);
  slots  entry k of a launch goes to slot ``length + k``, k = the number of set flags before (t, e) in row-major order of
         terminal [T,B]: by end step, then by env;
  capacity  an entry whose slot is >= capacity is not stored; ``length`` and ``carry`` advance as if it had been;
  cells  ``length += finished episodes``, ``step_base += T``; ``end_step = step_base (before) + t``.

Beside every running sum the model keeps how many terms it holds and the sum of their magnitudes: what a tolerance for a sum taken in
ANOTHER order is derived from (``pair_bound``).  The HIP kernel is compared with the model bit for bit and needs no tolerance.
"""
import numpy as np

from tests import episode_ledger_ref as elr

NOT_STORED = object()


def _planes(rew, terminal):
    """numpy or torch planes -> (rew as nested lists of Python floats, terminal as a bool array)."""
    if hasattr(rew, 'detach'):
        rew = rew.detach().cpu().numpy()
    if hasattr(terminal, 'detach'):
        terminal = terminal.detach().cpu().numpy()
    rew, term = np.asarray(rew), np.asarray(terminal)
    assert rew.dtype == np.float32 and rew.ndim == 3 and term.shape == rew.shape[:2], (rew.dtype, rew.shape, term.shape)
    return rew.astype(np.float64).tolist(), term != 0


class EpisodeLogModel(object):
    """The log as Python lists; the surface of ``train.EpisodeLog`` (``absorb`` / ``len`` / ``finished`` / ``entries`` / ``mean_of_last``
    / ``history``), so that it stands where one is used (``make_ledger=``).  ``device`` is accepted and ignored."""

    def __init__(self, num_envs, num_agents, capacity, device=None, carry=None, length=0, step_base=0):
        self.B, self.N, self.capacity = int(num_envs), int(num_agents), int(capacity)
        self.total = [NOT_STORED] * self.capacity
        self.by_agent = [[NOT_STORED] * self.N for _ in range(self.capacity)]
        self.end_step = [NOT_STORED] * self.capacity
        self.env = [NOT_STORED] * self.capacity
        self.carry = [[0.0] * (self.N + 1) for _ in range(self.B)] if carry is None else [[float(x) for x in row] for row in carry]
        assert len(self.carry) == self.B and all(len(r) == self.N + 1 for r in self.carry)
        self.length, self.step_base = int(length), int(step_base)
        # the derivation's side: terms and magnitudes of every running sum (a carried-in sum counts as one term)
        self.carry_terms = [[0 if x == 0.0 else 1 for x in row] for row in self.carry]
        self.carry_abs = [[abs(x) for x in row] for row in self.carry]
        self.terms, self.abs_sum = {}, {}                       # slot -> [N + 1] lists, for stored entries

    def absorb(self, rew, terminal):
        rew, term = _planes(rew, terminal)
        T, B, N = len(rew), self.B, self.N
        assert term.shape == (T, B) and len(rew[0]) == B and len(rew[0][0]) == N
        slot, k = {}, 0
        for t in range(T):                                      # (t, e) row-major: by end step, then by env
            for e in range(B):
                if term[t, e]:
                    slot[(t, e)] = self.length + k
                    k += 1
        for e in range(B):                                      # one env at a time, as run.py steps its one world
            by, n_terms, mags = self.carry[e], self.carry_terms[e], self.carry_abs[e]
            for t in range(T):
                for i, r in enumerate(rew[t][e]):               # run.py:55-57
                    by[N] += r
                    by[i] += r
                    n_terms[N] += 1
                    n_terms[i] += 1
                    mags[N] += abs(r)
                    mags[i] += abs(r)
                if term[t, e]:
                    s = slot[(t, e)]
                    if 0 <= s < self.capacity:
                        self.total[s], self.by_agent[s] = by[N], list(by[:N])
                        self.end_step[s], self.env[s] = self.step_base + t, e
                        self.terms[s], self.abs_sum[s] = list(n_terms), list(mags)
                    for i in range(N + 1):
                        by[i], n_terms[i], mags[i] = 0.0, 0, 0.0    # assignment: nothing of the old sum survives
        self.length += k
        self.step_base += T

    def finished(self):
        return self.length

    __len__ = finished

    def stored(self):
        return min(self.length, self.capacity)

    def entries(self):
        if self.length > self.capacity:
            raise RuntimeError('episode log overflowed: %d episodes finished, capacity %d' % (self.length, self.capacity))
        n = self.length
        assert all(x is not NOT_STORED for x in self.total[:n])
        return dict(total=np.array(self.total[:n], np.float64), by_agent=np.array(self.by_agent[:n], np.float64).reshape(n, self.N),
                    end_step=np.array(self.end_step[:n], np.int64), env=np.array(self.env[:n], np.int32))

    def mean_of_last(self, n, finished=None):
        tail = self.entries()['total'][-int(n):]
        return float(np.mean(tail)) if tail.size else float('nan')

    def history(self, include_open=True):
        ent = self.entries()
        totals = ent['total'].tolist()
        by_agent = [ent['by_agent'][:, i].tolist() for i in range(self.N)]
        if not include_open:
            return {'reward_episodes': totals, 'reward_episodes_by_agents': by_agent, 'open_episodes': 0,
                    'episode_end_step': ent['end_step'].tolist(), 'episode_env': ent['env'].tolist()}
        totals.extend(row[self.N] for row in self.carry)
        for i in range(self.N):
            by_agent[i].extend(row[i] for row in self.carry)
        return {'reward_episodes': totals, 'reward_episodes_by_agents': by_agent, 'open_episodes': self.B}

    def snapshot(self):
        """What a launch leaves, as arrays: the stored prefix of the four arrays, carry, length, step_base."""
        n = self.stored()
        filled = [s for s in range(n) if self.total[s] is not NOT_STORED]
        assert filled == list(range(filled[0], n)) if filled else True      # slots below the first launch's length stay untouched
        first = filled[0] if filled else n
        return dict(first=first, stored=n, total=np.array(self.total[first:n], np.float64),
                    by_agent=np.array(self.by_agent[first:n], np.float64).reshape(n - first, self.N),
                    end_step=np.array(self.end_step[first:n], np.int64), env=np.array(self.env[first:n], np.int32),
                    carry=np.array(self.carry, np.float64), length=self.length, step_base=self.step_base)


def pair_bound(terms, abs_sum):
    """How far two float64 sums of the same ``terms`` numbers may lie apart when each is taken in SOME order or tree, one rounding per
    addition: each is within gamma_(terms-1) * abs_sum of the exact sum (Higham, section 4.2; ``episode_ledger_ref.bound``'s source), so
    they are within 2 gamma_(terms-1) * abs_sum <= gamma_(2 terms) * abs_sum = bound(2 terms, abs_sum) of each other."""
    return elr.bound(2 * int(terms), float(abs_sum))


# ------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------
def synthetic_case(B, T, N, calls=3, seed=0, kinds=None, quantised=False):
    """Inputs for ``calls`` consecutive launches into one log, after ``episode_ledger_ref.synthetic_case``: dict(rew [calls,T,B,N]
    float32, terminal [calls,T,B] bool, carry0 [B,N+1] float64, length0, step_base0, kinds).  ``kinds[c]`` is 'mixed' (default), 'none' (no
    flag at all) or 'all' (every flag set: episodes of length 1).  What it guarantees (``assert_case_conditions`` checks it on the model
    alone), for the 'mixed' launches:
      - some env finishes no episode in the launch (B >= 2: in every one; B = 1: the last launch has no flag at all);
      - T >= 2: some env finishes two episodes inside one launch, the first on step 0 -- closing a carry that is not zero -- the second
        on the launch's last step;
      - the carry, the length and the step count start non-zero; column N of the carry is NOT the sum of the shares;
      - rewards of both signs with magnitudes from 1e-3 to 1e4 (log-uniform, both extremes present) -- or, ``quantised``: multiples of
        2**-10 with |r| <= 2**10 of both signs, whose float64 sums are exact in any order;
      - the ends are desynchronised: everywhere else a flag is an independent coin."""
    kinds = tuple(kinds) if kinds is not None else ('mixed',) * calls
    assert len(kinds) == calls and set(kinds) <= {'mixed', 'none', 'all'}
    rng = np.random.RandomState(1000003 * seed + 7919 * B + 131 * N + T)
    n = calls * T * B * N
    if quantised:
        rew = (rng.randint(-2 ** 20, 2 ** 20 + 1, n).astype(np.float64) * 2.0 ** -10).astype(np.float32)
        rew[0], rew[-1] = 2.0 ** -10, -(2.0 ** 10)
        carry0 = rng.randint(-2 ** 20, 2 ** 20, (B, N + 1)).astype(np.float64) * 2.0 ** -10 + 2.0 ** -10 * (B + 1)
    else:
        expo = rng.uniform(-3.0, 4.0, n)
        sign = np.where(rng.rand(n) < 0.5, -1.0, 1.0)
        expo[0], sign[0] = -3.0, 1.0
        expo[-1], sign[-1] = 4.0, -1.0
        rew = (sign * 10.0 ** expo).astype(np.float32)
        carry0 = np.where(rng.rand(B, N + 1) < 0.5, -1.0, 1.0) * 10.0 ** rng.uniform(-2.0, 3.0, (B, N + 1))
    rew = rew.reshape(calls, T, B, N)
    term = rng.rand(calls, T, B) < min(0.4, 2.5 / T)
    mixed = [c for c in range(calls) if kinds[c] == 'mixed']
    for c in range(calls):
        if kinds[c] != 'mixed':
            term[c] = kinds[c] == 'all'
            continue
        if B >= 2:
            quiet, busy = (B - 1, 0) if c % 2 == 0 else (0, B - 1)
            term[c, :, quiet] = False
        else:
            busy = 0
            if c == mixed[-1] and len(mixed) > 1:
                term[c] = False
                continue
        term[c, 0, busy] = True
        term[c, T - 1, busy] = True
    return dict(rew=rew, terminal=term, carry0=carry0, length0=41, step_base0=1000, kinds=kinds, quantised=quantised)


def run_model(case, capacity, calls=None):
    """-> (model after the last launch, [snapshot after each launch])."""
    _, T, B, N = case['rew'].shape
    m = EpisodeLogModel(B, N, capacity, carry=case['carry0'], length=case['length0'], step_base=case['step_base0'])
    snaps = []
    for c in range(case['rew'].shape[0] if calls is None else calls):
        m.absorb(case['rew'][c], case['terminal'][c])
        snaps.append(m.snapshot())
    return m, snaps


def capacity_for(case):
    """Room for every episode of the case behind ``length0``."""
    return int(case['length0'] + case['terminal'].sum())


def assert_case_conditions(case):
    """The guarantees of ``synthetic_case``, asserted on the model alone."""
    rew, term, kinds = case['rew'], case['terminal'], case['kinds']
    calls, T, B, N = rew.shape
    per_env = term.sum(1)                                     # [calls, B]
    mixed = [c for c in range(calls) if kinds[c] == 'mixed']
    for c in range(calls):
        if kinds[c] == 'none':
            assert not term[c].any()
        if kinds[c] == 'all':
            assert term[c].all()
    assert mixed, 'a case needs a mixed launch'
    assert (per_env[mixed] == 0).any(), 'no env without a finished episode'
    if B >= 2:
        assert (per_env[mixed] == 0).any(1).all() and (per_env[mixed] > 0).any(1).all()
    if T >= 2:
        twice = (per_env[mixed] >= 2) & term[mixed, 0, :] & term[mixed, T - 1, :]
        assert twice.any(), 'no env finishes on step 0 and again on the last step of one launch'
    carry0 = np.asarray(case['carry0'])
    assert (carry0 != 0).all() and case['length0'] != 0 and case['step_base0'] != 0
    assert not np.any(carry0[:, N] == carry0[:, :N].sum(1))
    assert kinds[0] != 'mixed' or term[0, 0].any()
    # the carry is part of the first entry: the model run from a zero carry stores another first entry
    m, _ = run_model(case, capacity_for(case), calls=1)
    z = EpisodeLogModel(B, N, capacity_for(case), length=case['length0'], step_base=case['step_base0'])
    z.absorb(rew[0], term[0])
    if term[0].any():
        s = case['length0']
        assert m.total[s] != z.total[s] and m.by_agent[s] != z.by_agent[s]
        assert (m.end_step[s], m.env[s]) == (z.end_step[s], z.env[s]) == (case['step_base0'] + int(np.argwhere(term[0])[0][0]),
                                                                          int(np.argwhere(term[0])[0][1]))
    a = np.abs(rew.astype(np.float64))
    assert (rew > 0).any() and (rew < 0).any()
    if case['quantised']:
        assert a.max() <= 2.0 ** 10 and np.array_equal(rew.astype(np.float64) * 2.0 ** 10, np.round(rew.astype(np.float64) * 2.0 ** 10))
        assert np.array_equal(carry0 * 2.0 ** 10, np.round(carry0 * 2.0 ** 10))
    else:
        assert 0.999e-3 <= a.min() <= 1.001e-3 and 0.999e4 <= a.max() <= 1.001e4       # seven decades
    if B >= 8:
        assert len(set(per_env[mixed[0]].tolist())) > 1       # not every env ends at once
