"""CPU: tests/update_ref.py itself -- the staged restatement of one learner update, its recorder and its check.

1. The restatement is the learner's algorithm: free-running in float64 (its own picks, its own post-step critic, its own gradients)
   it equals examples/madr_learner.py's three classes on the CPU in float64, ``_sample`` replaced by ``sampling_ref.stock`` on the same
   noise, in every named quantity of 3 updates, to 1e-10 relative to the quantity's largest entry (the same mathematics in another
   summation order; Adam's early step magnifies a float64 rounding of a gradient by at most 1 / eps = 1e8).
2. The harness end to end without a GPU: a float32 learner with every network switch on -- the launches replaced by the restatement
   stand-ins of test_head_host.py, lstm_wgrad_ref.py and sampling_ref.py -- the stock optimiser and module targets passes
   ``update_ref.check_case`` with the recorder installed.
3. The check would fail if the update were subtly wrong: a float32 restatement that does the update wrongly in one way plays the
   learner; ``check_case`` must name a failure for every mutation, and none for the unmutated player.
"""
import os
import sys

import pytest

torch = pytest.importorskip('torch')

from tests import lstm_wgrad_ref, sampling_ref, update_ref  # noqa: E402
from tests.test_head_host import standins  # noqa: E402,F401  (the fixture: the network launches replaced by restatements)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = ['attention', 'two_head', 'bicnet', 'model']
SEED = 5


def _madr_learner():
    if os.path.join(ROOT, 'examples') not in sys.path:
        sys.path.insert(0, os.path.join(ROOT, 'examples'))
    import madr_learner
    return madr_learner


def _learner(variant, dtype, batch, weights_seed=3, **switches):
    meta = update_ref.make_meta(variant, SEED)
    torch.manual_seed(weights_seed)
    actor, critic = meta['make_actor']().to(dtype), meta['make_critic']().to(dtype)
    ring = update_ref.HostRing(variant)
    t = getattr(_madr_learner(), meta['cls'])(actor, critic, ring, action_type='MultiDiscrete' if len(ring.heads) == 2 else 'Discrete',
                                              batch_size=batch, device='cpu', **switches)
    return t, meta


def _rel(x, y):
    return float((x.double() - y.double()).abs().max()) / max(float(y.double().abs().max()), 1e-300)


# ---- 1. the restatement is the learner's algorithm -----------------------------------------------------------------------------------
@pytest.mark.parametrize('variant', VARIANTS)
def test_free_running_restatement_equals_the_learner_in_float64(variant, monkeypatch):
    t, meta = _learner(variant, torch.float64, 9)
    as_tensor = torch.as_tensor   # the learner asks for its batch in float32 by name: in this test that name means float64
    monkeypatch.setattr(torch, 'as_tensor', lambda x, dtype=None, device=None: as_tensor(
        x, dtype=torch.float64 if dtype == torch.float32 else dtype, device=device))
    sampler = t._sample = update_ref.StockSampler(SEED)
    rec = update_ref.Recorder(t, meta)
    mine = None
    for u in range(3):
        t.optimize()
        sampler.end_update()
        got = rec.records[u]
        if mine is None:
            mine = update_ref.Restatement(got['meta'], got['pre'], torch.float64, 'cpu')   # with what the recorder adds: a stock optimiser
        want = mine.update(got['batch'], u)
        a, b = update_ref.named(got), update_ref.named(want)
        assert set(a) == set(b) and len(a) > 60
        for n in b:
            assert a[n].numel() == b[n].numel() and _rel(a[n].reshape(-1), b[n].reshape(-1)) <= 1e-10, (variant, u, n)
        assert float(b['C.total_norm']) > 0 and float(b['D.grad.' + meta['names']['actor'][0]].abs().max()) > 0
        assert len(got['sites']) == len(want['sites']) == 2 * len(t.memory.heads)
        for s, w in zip(got['sites'], want['sites']):
            assert torch.equal(s['pick'].view(-1), w['pick'].view(-1))
        for x, y in zip(update_ref.state_tensors(got['post']), update_ref.state_tensors(want['post'])):
            assert _rel(x, y) <= 1e-10
    assert rec.records[2]['pre']['critic_opt']['step'] == [2.0] * len(meta['names']['critic'])


# ---- 2. the harness end to end on stand-ins ------------------------------------------------------------------------------------------
@pytest.fixture
def all_standins(standins, monkeypatch):  # noqa: F811
    from multiagent_rl_amd import lstm, sampling
    monkeypatch.setattr(lstm, 'launch_wgrad', lstm_wgrad_ref.launch_wgrad)
    monkeypatch.setattr(sampling, 'launch_forward', sampling_ref.launch_forward)
    monkeypatch.setattr(sampling, 'launch_backward', sampling_ref.launch_backward)
    monkeypatch.setattr(sampling, 'launch_advance', sampling_ref.launch_advance)
    return standins


@pytest.mark.parametrize('variant', VARIANTS)
def test_an_all_switches_learner_on_stand_ins_passes_the_check(all_standins, variant):
    t, meta = _learner(variant, torch.float32, 9, fused_lstm=True, fused_attention=True, fused_sampling=True, sampling_seed=SEED,
                       fused_front=True, fused_wgrad=True, fused_heads=True)
    assert t.actor.fused_heads and t.critic.fused_heads and t.target_critic.fused_heads and not t.fused_optimizer
    rec = update_ref.Recorder(t, meta)
    del all_standins.calls[:]
    for u in range(3):
        t.optimize()
        assert int(t.sampler.cell) == 16 * (u + 1)
    assert all_standins.calls                                              # the fused forwards ran: the stand-ins were called
    assert len(rec.records) == 3 and all(len(r['sites']) == 2 * len(t.memory.heads) for r in rec.records)
    for before, after in zip(rec.records, rec.records[1:]):               # nothing else wrote between two updates
        assert all(update_ref.same_bits(x, y) for x, y in zip(update_ref.state_tensors(before['post']), update_ref.state_tensors(after['pre'])))
    lines = []
    fails, worst = update_ref.check_case('%s stand-ins b 9' % variant, rec.records, 'cpu', report=lines.append)
    print('\n'.join(lines))
    assert not fails, fails
    assert sorted(worst) == ['A', 'B', 'C', 'D', 'E'] and len(lines) == 15 + (variant == 'model')


# ---- 3. every mutation is caught -----------------------------------------------------------------------------------------------------
def _played(variant, mutate, updates=3, batch=9):
    meta = update_ref.make_meta(variant, SEED)
    player = update_ref.Restatement(meta, update_ref.initial_state(meta, 3), torch.float32, 'cpu')
    ring = update_ref.HostRing(variant)
    return [player.update(ring.sample_index(ring.make_index(batch)), u, mutate=mutate) for u in range(updates)]


def _variant_of(mutation):
    return {'L1 term dropped': 'model', 'y from the agent-mean reward': 'bicnet'}.get(mutation, 'attention')


@pytest.mark.parametrize('variant', VARIANTS)
def test_the_unmutated_player_passes(variant):
    fails, worst = update_ref.check_case('%s honest player' % variant, _played(variant, None), 'cpu', report=lambda line: None)
    assert not fails, fails
    assert max(worst.values()) <= 1.0, worst                               # the yardstick's own arithmetic


@pytest.mark.parametrize('mutation', update_ref.MUTATIONS)
def test_a_mutated_update_is_caught(mutation):
    fails, _ = update_ref.check_case(mutation, _played(_variant_of(mutation), mutation), 'cpu', report=lambda line: None)
    print('%s:\n  %s' % (mutation, '\n  '.join(fails[:6])))
    ratios = [f for f in fails if 'ratio' in f]
    assert ratios, (mutation, fails)                                       # a named quantity beyond the bound, not only a pick
