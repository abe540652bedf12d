"""GPU: the learner's whole update with every fused switch on -- ``madr_learner``'s ``optimize_tensors`` on the HIP kernels of the
no-grad half, the LSTMs, the attention, the sampler, the dense front, dW_hh, the heads and the optimiser tail -- held, quantity by
quantity and update by update, to the staged float64 restatement of tests/update_ref.py.

The learner is test_gpu_heads._learner's (eager, every switch, sampler seed 5, ``accelerate_trainer(targets=True)``, a
``device_index='counter'`` ring, the default lr 1e-2) at the batch size of the case.  Per update, from the recorder's record:

* every named quantity of stages (A) to (E) within the project's bound: |learner - float64| <= 4 x max(|stock float32 on the GPU -
  float64|, one float32 rounding of the reference's largest entry); total_norm within 2e-6 relative (test_gpu_optim.py's);
* the pick check: the learner's pick is the float64 argmax wherever the float64 margin is at least twice the logits' disagreement;
* the pre-update state of update u + 1 has the bits of what the two steps of update u left, and the sampler's cell reads 16 (u + 1);
* the recorder changes nothing: a second learner from the same weights, without it, has the same bits in every tensor after every
  update -- which ties what is checked here to what the bit-for-bit graph tests pin.

Measured on an MI355X (profiles/update_parity.txt), largest ratio per stage over all cases: A 3.59, B 2.18, C 1.57, D 2.20, E 1.17;
no row of any site under the pick check's margin; the model variant's least L1 distance 6.4e-4.

What this test found: with the training LSTM's cell on fast_tanh (2 / (1 + e) - 1: one rounding of 1, ~1e-7 absolute, whatever the
value) two_head-b33 failed in update 0 at ``B.grad.dense2.weight`` (the critic's): learner 7.206e-09, stock 1.450e-09, ratio 4.97.
Not stage (A) (same figures on the learner's own y), not the heads' sums (``pw_head_train_backward`` on that pass's operands had
torch's float32 matmul's error to the digit); 7.0e-9 of it was the context's error, already in the LSTM output (rms 2.8e-08 against
MIOpen's 8.1e-09, mean +3.4e-09 against 1.4e-10), which a sum over rows against a dOut of mostly one sign keeps.  The cell of the
kernels with gradient now takes tanhf (csrc/pw_kernels_lstm.hpp, lstm_cell_train): that ratio is 1.76, and
test_gpu_lstm_train.py::test_small_outputs_keep_their_relative_accuracy is the kernel-level case.

``PW_UPDATE_PARITY_REPORT=<path>``: every case appends its lines there (profiles/update_parity.txt is where such a run is kept).
"""
import copy
import os

import pytest
import torch

from tests import update_ref

pytestmark = pytest.mark.gpu

# batch 5: 15 rows, the heads' single-launch backward and less than a tile; 683: 2049 rows at N = 3, the first count at which a
# workgroup owns two 16-row tiles
CASES = [('attention', 33), ('two_head', 33), ('bicnet', 33), ('model', 33), ('attention', 5), ('attention', 683)]
UPDATES, SEED = 4, 5


def _report(line):
    print(line)
    path = os.environ.get('PW_UPDATE_PARITY_REPORT')
    if path:
        with open(path, 'a') as f:
            f.write(line + '\n')


def _learner(ug, variant, nets, batch):
    import madr_learner
    from multiagent_rl_amd.policy import accelerate_trainer
    cls_name, _, _, ring_kw, N, D = ug.VARIANTS[variant]
    actor, critic = copy.deepcopy(nets)
    t = getattr(madr_learner, cls_name)(actor, critic, ug._filled_memory(ring_kw, N, D),
                                        action_type='MultiDiscrete' if 'act_heads' in ring_kw else 'Discrete', batch_size=batch,
                                        fused_optimizer=True, fused_lstm=True, fused_attention=True, graph_update=False,
                                        fused_sampling=True, sampling_seed=SEED, fused_front=True, fused_wgrad=True, fused_heads=True)
    accelerate_trainer(t, targets=True)
    return t


@pytest.mark.parametrize('variant,batch', CASES, ids=['%s-b%d' % c for c in CASES])
def test_every_stage_of_the_fused_update_against_float64(variant, batch):
    import tests.test_gpu_update_graph as ug                              # the harness: VARIANTS, _filled_memory, _everything, _same
    from multiagent_rl_amd import critic as cr, policy as pol
    from multiagent_rl_amd.critic import _FusedTarget
    from multiagent_rl_amd.optim import FusedAdam
    torch.manual_seed(3)
    nets = (ug.VARIANTS[variant][1](pol, cr), ug.VARIANTS[variant][2](pol, cr))
    a, b = _learner(ug, variant, nets, batch), _learner(ug, variant, nets, batch)
    assert isinstance(a.critic_optimizer, FusedAdam) and isinstance(a.target_critic, _FusedTarget) and a.actor.fused_heads
    assert float(a.critic_optimizer.param_groups[0]['lr']) == 1e-2
    rec = update_ref.Recorder(a, update_ref.make_meta(variant, SEED))
    for u in range(UPDATES):
        la, lb = a.optimize(), b.optimize()
        assert int(a.sampler.cell) == 16 * (u + 1)
        sa, sb = ug._everything(a), ug._everything(b)
        bad = [i for i, (x, y) in enumerate(zip(sa, sb)) if not ug._same(x, y)]
        assert la == lb and len(sa) > 20 and not bad, (variant, batch, u, la, lb, bad[:5])           # the recorder changes nothing
    records = rec.records
    assert len(records) == UPDATES and all(r['batch'][0].shape[0] == batch for r in records)
    for u, r in enumerate(records):
        assert bool(torch.isfinite(r['loss_actor'])) and bool(torch.isfinite(r['loss_critic'])) and len(r['sites']) == (4 if variant == 'two_head' else 2)
        for net in ('critic', 'actor'):                                   # the state after the update is what the two steps left ...
            step, post = r[net + '_step'], r['post']
            left = step['params'] + step['targets'] + step['exp_avg'] + step['exp_avg_sq']
            after = post[net] + post['target_' + net] + post[net + '_opt']['exp_avg'] + post[net + '_opt']['exp_avg_sq']
            assert all(update_ref.same_bits(x, y) for x, y in zip(left, after)), (variant, batch, u, net)
            assert post[net + '_opt']['step'] == [float(u + 1)] * len(step['params'])
        if u:                                                             # ... and what the next update starts from: nothing else wrote
            before = update_ref.state_tensors(records[u - 1]['post'])
            assert all(update_ref.same_bits(x, y) for x, y in zip(before, update_ref.state_tensors(r['pre']))), (variant, batch, u)
    fails, worst = update_ref.check_case('%s b %d' % (variant, batch), records, 'cuda', report=_report)
    _report('%s b %d: worst ratio per stage over %d updates: %s' % (variant, batch, UPDATES, '  '.join(
        '%s %.2f' % (s, worst[s]) for s in sorted(worst))))
    assert not fails, '\n'.join(fails)
    assert sorted(worst) == ['A', 'B', 'C', 'D', 'E']
