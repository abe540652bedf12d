"""-m gpu: TWO processes sharing GPU 0 -- the BiCNet baseline's multi-rank path with the product's HIP launches in every rank.

As tests/test_gpu_two_ranks.py (whose ``_launch`` this uses: fresh child processes, a gloo group, the blocks of the full gather staged
through pinned host buffers), with ``FullTransitionGather(per_agent=True)``: every block travels with its trailer plane and the root
appends with the ``pw_replay_add_*wire_agents`` launches.  Each test is one launch of two children, each child under the launch's
time limit; a child that fails ends its test, and nothing further is started in it."""
import json
import os
import pickle

import numpy as np
import pytest

from tests.test_gpu_two_ranks import _launch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, 'tests', 'per_agent_two_rank_worker.py')
pytestmark = pytest.mark.gpu


@pytest.mark.timeout(400)
def test_per_agent_full_gather_of_two_ranks_fills_the_root_ring_rank_by_rank():
    """State blocks -> per-agent STATE ring (simple_spread N = 6, simple_tag 4 + 2), row blocks -> per-agent row ring, simple_reference's
    compact rows -> per-agent two-head ring, 4 chunks each (the three block slots wrap): the root's ring holds rank r's chunk x at
    [(x*2 + r)*T*B, +T*B), bit-identical to the per-agent ring rank r's own rollout sink fills -- rew / done [., N] included."""
    out = _launch(2, [WORKER], timeout=300)
    res = [json.loads(l) for l in out.splitlines() if l.startswith('{')]
    assert [r['case'] for r in res] == ['spread_state_ring', 'spread_row_blocks', 'tag_state_ring', 'reference_two_head']
    assert all(r['ok'] and r['world'] == 2 and r['transitions_with_distinct_rewards'] > 0 for r in res)
    by = {r['case']: r for r in res}
    assert by['spread_state_ring']['wire'] == 'state' and by['spread_row_blocks']['wire'] == 'rows' and by['reference_two_head']['wire'] == 'ref'
    assert by['spread_state_ring']['transitions'] == 2 * 4 * 40 * 96
    # 21 N + 5 bytes per env-step and the per-chunk planes (T = 40: two episode ends per env) against the shared block's 17 N + 5
    assert 131 < by['spread_state_ring']['bytes_per_env_step'] < 160


@pytest.mark.timeout(400)
def test_bicnet_entry_script_on_two_ranks_sharing_the_gpu(tmp_path):
    """examples/train_batched.py --backend gloo --critic bicnet --fused-targets as two ranks, at the size of
    test_entry_script_on_two_ranks_sharing_the_gpu: both ranks roll out into per-agent wire blocks, rank 0 owns the per-agent STATE ring and
    the BiCNet learner."""
    out = _launch(2, [WORKER, 'entry', '--backend', 'gloo', '--scenario', 'simple_spread', '--envs', '256', '--agents', '3',
                      '--episodes', '1024', '--chunk', '50', '--save-rate', '512', '--max-updates-per-chunk', '3', '--critic', 'bicnet',
                      '--fused-targets', '--out-dir', str(tmp_path / 'Models')], cwd=str(tmp_path), timeout=300)
    assert 'simple_spread cnt=0: 25600 env-steps, 1024 episodes' in out, out[-2000:]                 # the run finished
    rep = [json.loads(l) for l in out.splitlines() if l.startswith('{')][-1]
    st = rep['stats']
    assert st['world'] == 2 and st['updates_run'] == 3 and st['updates'] == 3                         # updates ran
    assert rep['learner'] and rep['per_agent'] and rep['state_ring']                                  # a per-agent STATE ring
    assert rep['rew_shape'][1] == 3 and rep['filled'] == 2 * 25600                                   # both ranks' two chunks of 256 x 50
    hist = pickle.load(open(tmp_path / 'Models' / 'history_simple_spread_0.pkl', 'rb'))
    assert hist['episodes_per_rank'] == [1024 + 256, 1024 + 256] and len(hist['reward_episodes_by_agents']) == 3
    assert np.isfinite(hist['reward_episodes']).all() and all(np.isfinite(x).all() for x in hist['reward_episodes_by_agents'])
    assert os.path.exists(tmp_path / 'Models' / 'simple_spread_fin_0_actor.pt')
