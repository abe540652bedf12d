"""CPU: the float32 C oracle against the float64 C oracle FREE-RUNNING over four whole 25-step episodes with auto-reset
(T = 100) -- what the single-step parity tests never see: how far float32 drifts along a trajectory, and that resets, episode
clocks and masks chain identically in both precisions.

Only what follows from the construction is asserted (tests/trajectory.py: check_reset, check_clocks, check_mask_flips,
check_rewards, check_contact_free); no drift figure is typed in.  The figures are printed and, with PW_TRAJECTORY_REPORT=<path>,
appended to that file (profiles/trajectory_drift.txt holds such a run).

Coverage conditions (on the inputs, judged on the float64 side): every colliding scenario's case holds env-steps with and without a
contact so far in the episode, except N >= 24 where contact-free ones may be absent (from N = 9 upwards they are a handful
of envs in their first steps: see the seed note in tests/trajectory.py); the two communication scenarios have
no colliding entity at all, so every env of theirs is contact-free by construction; at least one case crosses 1e-5.
"""
import numpy as np
import pytest

from tests import trajectory as tj

drift_of = tj.oracle_drift       # one float32-vs-float64 run per case, shared by every test here (and read-only)


@pytest.mark.parametrize('case', tj.CASES, ids=[c['id'] for c in tj.CASES])
def test_float32_oracle_free_running_against_float64(case):
    d = drift_of(case)
    assert d.T == 100 and d.term.sum() == 4 * d.B
    info = tj.check_structure(d)
    tj.report(tj.table(d, 'cpu float32 C oracle vs float64 C oracle: ' + case['id']) + [tj.summary_line(case['id'], info)])
    assert info['resets'] == 5 and info['reset_states'] == 5
    if d.comm:
        assert not d.contact.any()                              # nobody collides in these worlds
    else:
        assert info['contact_env_steps'] > 0
        assert info['free_env_steps'] > 0 or case['num_agents'] >= 24
        # the masks must have seen real contacts, not only the self bits
        self_bits = (np.uint64(1) << np.arange(d.N, dtype=np.uint64))[None, None, :]
        assert (d.ref['coll'] != self_bits).any()


def test_some_case_leaves_the_single_step_tolerance():
    """The sentence 'within 1e-5 of the float64 oracle' holds for a step, not for an episode: at least one case must cross it
    (a condition on the chosen seeds and shapes, so that the structural assertions are exercised beyond the tolerance)."""
    crossed = [case['id'] for case in tj.CASES if tj.horizon(drift_of(case))[0] is not None]
    assert crossed, 'no case crossed 1e-5: choose seeds that do'


def test_report_figures_are_split_by_contact():
    """The helper's figures: per step, the groups partition the batch and 'all' is the worse of the two."""
    d = drift_of(tj.CASES[1])
    fig = tj.figures(d)
    assert len(fig) == d.T and [r['s'] for r in fig[:26]] == list(range(25)) + [0]
    for r in fig:
        assert r['n_contact'] + r['n_free'] == d.B
        parts = [r[g + '_obs'][0] for g in ('contact', 'free') if not np.isnan(r[g + '_obs'][0])]
        assert r['all_obs'][0] == max(parts)
        assert 0.0 <= r['all_obs'][3] <= 1.0 and r['all_obs'][2] <= r['all_obs'][1] <= r['all_obs'][0]
    # contact is monotone within an episode and starts afresh at each reset
    c = d.contact.reshape(tj.EPISODES, tj.EP_LEN, d.B)
    assert (c[:, 1:] >= c[:, :-1]).all()
