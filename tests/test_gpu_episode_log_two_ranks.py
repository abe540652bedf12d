"""-m gpu: two processes sharing GPU 0 train with ``--ledger device`` (the pattern of tests/test_gpu_two_ranks.py: a gloo group, the blocks of
the full gather through pinned host buffers, the product's HIP launches in both ranks).  Each rank's episode log absorbs the rew / terminal
side buffers of its gather; rank 0 merges the two histories in time order.  One child-process pair, under its own time limit."""
import os
import pickle
import socket
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _free_port():
    sk = socket.socket()
    sk.bind(('127.0.0.1', 0))
    port = sk.getsockname()[1]
    sk.close()
    return port


def _launch(world, argv, cwd, timeout=300):
    """`world` ranks of `argv` (RANK / WORLD_SIZE / MASTER_* in the env), all on GPU 0; returns rank 0's stdout."""
    port = _free_port()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port),
                   PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
        procs.append(subprocess.Popen([sys.executable] + argv, cwd=cwd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    outs = []
    try:
        for p in procs:
            outs.append(p.communicate(timeout=timeout))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for r, (p, (so, se)) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, 'rank %d exited %s\n%s\n%s' % (r, p.returncode, so[-2000:], se[-4000:])
    return outs[0][0]


@pytest.mark.timeout(400)
def test_two_ranks_merge_their_episode_logs_in_time_order(tmp_path):
    """examples/train_batched.py --backend gloo --ledger device as two ranks of 256 envs, 50-step chunks, 1024 episodes per rank: the
    pickled history lists the finished episodes of both ranks by (end step, rank, env) with the rank and the global env id beside
    each, then the 512 open returns in global env order, under ONE open count."""
    B = 256
    out = _launch(2, [os.path.join(ROOT, 'examples', 'train_batched.py'), '--backend', 'gloo', '--scenario', 'simple_spread', '--envs', str(B),
                      '--agents', '3', '--episodes', '1024', '--chunk', '50', '--save-rate', '512', '--max-updates-per-chunk', '3',
                      '--ledger', 'device', '--out-dir', str(tmp_path / 'Models')], cwd=str(tmp_path))
    assert 'simple_spread cnt=0: 25600 env-steps, 1024 episodes' in out, out[-2000:]
    hist = pickle.load(open(tmp_path / 'Models' / 'history_simple_spread_0.pkl', 'rb'))
    n = 2 * 1024
    assert hist['episodes_per_rank'] == [1024, 1024] and hist['open_episodes'] == 2 * B and hist['stats']['world'] == 2
    assert len(hist['reward_episodes']) == n + 2 * B and [len(x) for x in hist['reward_episodes_by_agents']] == [n + 2 * B] * 3
    steps, ranks, envs = (np.array(hist[k]) for k in ('episode_end_step', 'episode_rank', 'episode_env'))
    assert len(steps) == len(ranks) == len(envs) == n
    # every env's episode is 25 steps from a common reset: the ends are the steps 24, 49, 74, 99, each with all 512 worlds in
    # (rank, env) order -- global env id ascending
    assert np.array_equal(steps, np.repeat([24, 49, 74, 99], 2 * B))
    assert np.array_equal(envs, np.tile(np.arange(2 * B), 4)) and np.array_equal(ranks, envs // B)
    tot, by = np.array(hist['reward_episodes']), np.array(hist['reward_episodes_by_agents'])
    assert np.isfinite(tot).all() and (tot[:n] < 0).all()
    # the total is a float64 sum of its own over the same float32 rewards as the shares: equal to their sum within gamma_76 of the 75 terms' magnitudes, each way (all rewards are <= 0)
    assert np.abs(tot - by.sum(0)).max() <= 2.0 ** -53 * 2 * 76 * np.abs(tot).max()
    # the two ranks are different worlds (env_id_base): their first episodes differ; the open returns are fresh episodes (just reset)
    assert not np.array_equal(tot[:B], tot[B:2 * B]) and not tot[n:].any()
    assert os.path.exists(tmp_path / 'Models' / 'simple_spread_fin_0_actor.pt')
