"""CPU, two gloo ranks: ``train.evaluate_batched(world=2)`` with the stubs of tests/test_episode_log_host.py and the model as the log --
every rank plays its own envs, rank 0 gathers the histories and merges them in time order, only rank 0 writes the file."""
import os
import pickle
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from multiagent_rl_amd.train import evaluate_batched, merge_histories_chronological
from tests import episode_log_ref as ref
from tests import test_episode_log_host as host


def _free_port():
    sk = socket.socket()
    sk.bind(('127.0.0.1', 0))
    port = sk.getsockname()[1]
    sk.close()
    return port


class _RankFused(host._StubFused):
    """Rank r's worlds run r + 1 steps ahead of rank 0's: the two ranks' episode ends interleave."""

    def __init__(self, trace, rank):
        super().__init__(trace)
        self.rank = rank

    def rollout(self, env, num_steps, out=None, memory=None, stats=None):
        rew, term = host._stub_planes(self.steps + (self.rank + 1) * self.rank, num_steps, env.num_envs, env.n)
        out['rew'].copy_(rew - 100.0 * self.rank)
        out['terminal'].copy_(term)
        self.steps += num_steps
        stats[2].add_(int(term.sum()))
        return out


def _run(rank, world, out_dir):
    trace = []
    host._StubTrainer.trace = trace
    env = host._StubEnv()
    hist = evaluate_batched(env, 'actor', 'critic', host._StubTrainer, 'simple_spread', 'Discrete', cnt=2, arglist=host._Args(), out_dir=out_dir,
                            log=lambda *a: None, make_ledger=ref.EpisodeLogModel, rank=rank, world=world,
                            make_rollout=lambda e, actor, memory, seed: (_RankFused(trace, rank), host._StubRollout(e, memory, trace)))
    return hist, trace


def _worker(rank, world, port, out_dir, q):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    hist, trace = _run(rank, world, out_dir)
    q.put(dict(rank=rank, hist=hist, kinds=[e[0] for e in trace]))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(180)
def test_evaluate_batched_over_two_ranks(tmp_path):
    if torch.cuda.device_count() > 0:
        pytest.skip('CPU-container test: it spawns worker processes')
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, str(tmp_path), q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=120) for _ in range(2)], key=lambda r: r['rank'])
    for p in procs:
        p.join(30)
        assert p.exitcode == 0
    r0, r1 = res
    assert 'optimize' not in r0['kinds'] + r1['kinds'] and 'save_models' not in r0['kinds'] + r1['kinds']
    assert os.listdir(tmp_path) == ['test_history_simple_spread_2.pkl']          # rank 0 alone writes
    solo = []
    for r in range(2):                                                           # the same shards, one rank at a time
        h, _ = _run(r, 1, None)
        solo.append(dict({k: v for k, v in h.items() if k != 'stats'}, num_envs=8))
    want = merge_histories_chronological(solo)
    got = r0['hist']
    for k in want:
        assert got[k] == want[k], k
    assert sorted(got) == sorted(list(want) + ['stats']) and got['stats']['world'] == 2 and got['open_episodes'] == 0
    n = len(got['reward_episodes'])
    assert got['episodes_per_rank'] == [24, 24] and n == 48 and got['episode_end_step'] == sorted(got['episode_end_step'])
    assert set(got['episode_rank']) == {0, 1} and got['episode_rank'] != sorted(got['episode_rank'])      # interleaved, not concatenated
    assert all(got['reward_episodes'][k] <= -100.0 for k in range(n) if got['episode_rank'][k] == 1)
    assert all(got['episode_env'][k] // 8 == got['episode_rank'][k] for k in range(n))
    assert pickle.load(open(tmp_path / 'test_history_simple_spread_2.pkl', 'rb'))['reward_episodes'] == got['reward_episodes']
    # rank 1 keeps its own, unmerged history
    assert 'episode_rank' not in r1['hist'] and len(r1['hist']['reward_episodes']) == 24
