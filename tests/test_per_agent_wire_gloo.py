"""CPU, world_size 2, gloo: ``FullTransitionGather(per_agent=True)`` -- the per-agent reward plane travels as a trailer behind every wire
block.  Two ranks fill the root's per-agent ring rank by rank over FOUR chunks (the three block slots wrap), on the state-only blocks
into a row ring and (host transport) into a STATE ring, and on simple_reference's compact rows; what arrives of rank 1's ``rew`` planes
is what rank 1's "rollout" wrote, bit for bit.  The HIP launches are the torch stand-ins of tests/per_agent_standins.py (built on
tests/dist_standins.py); their GPU parity is in tests/test_gpu_per_agent_wire.py."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.per_agent_standins import CpuPerAgentGather
from tests.test_dist_gloo import (B, N, T, _free_port, _RefEnv, _SpreadEnv, episode_number, landmarks_of, ref_chunk, ref_obs0, spread_chunk,
                                  spread_start)

CHUNKS = 4


def agent_rewards(rank, k, n):
    """The per-agent rewards rank's rollout 'wrote' in chunk k: distinct per (rank, chunk, step, env, agent)."""
    g = torch.Generator()
    g.manual_seed(90210 + 1000 * rank + k)
    return torch.randn(T, B, n, generator=g)


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    res = {}
    for name, kw in (('rows_ring', {}), ('state_ring', dict(ring='state', transport='host'))):
        env = _SpreadEnv(rank)
        g = CpuPerAgentGather(env, T, rank, world, 'cpu', per_agent=True, **kw)
        assert g.per_agent and g.state_wire and g.side['rew'] is None and g.transport == kw.get('transport', 'direct')
        assert all(w.numel() == g.block_bytes == g.lay.total_bytes + 256 * -(-4 * T * B * N // 256) for w in g.wire)
        state0, lm0, ep0 = spread_start(rank)
        for k in range(CHUNKS):
            src = spread_chunk(rank, k, k * T)
            src['rew'] = agent_rewards(rank, k, N)
            env.start = (state0, lm0, ep0)
            out = g.outputs()
            assert out['rew'].data_ptr() == g.wire[k % 3].data_ptr() + g.lay.total_bytes        # a view INTO the block's trailer
            for nm in ('obs', 'rew_shared', 'terminal', 'act', 'final_obs', 'rew'):
                out[nm].copy_(src[nm])               # "the rollout kernel wrote its outputs"
            g(None)
            e = torch.arange(B)
            state0, ep0 = src['obs'][T - 1][..., :4].clone(), episode_number(e, (k + 1) * T)
            lm0 = landmarks_of(rank, e, ep0)
        g.finish()
        dist.barrier()
        if rank == 0:
            assert getattr(g.memory, 'per_agent', False)
            if name == 'state_ring':
                n = len(g.memory)
                res[name] = (g.rows_ingested, [x.numpy() for x in g.memory.sample_index(list(range(n)))])
            else:
                res[name] = (g.rows_ingested, [{kk: vv.numpy() for kk, vv in tr.items() if kk in ('obs', 'next_obs', 'act', 'rew', 'done')}
                                               for tr in g.memory.transitions])
    rg = CpuPerAgentGather(_RefEnv(), T, rank, world, 'cpu', per_agent=True)
    assert rg.ref_wire and rg.per_agent
    obs0 = ref_obs0(rank)
    for k in range(CHUNKS):
        src = ref_chunk(rank, k, k * T)
        src['rew'] = agent_rewards(rank, k, 2)
        out = rg.outputs()
        for nm in ('obs', 'rew_shared', 'terminal', 'act', 'final_obs', 'rew'):
            out[nm].copy_(src[nm])
        rg(obs0)
        obs0 = src['obs'][T - 1].clone()
    rg.finish()
    dist.barrier()
    if rank == 0:
        res['ref'] = (rg.rows_ingested, [{kk: vv.numpy() for kk, vv in tr.items()} for tr in rg.memory.transitions])
    q.put(res if rank == 0 else None)
    dist.destroy_process_group()


@pytest.fixture(scope='module')
def root():
    if torch.cuda.device_count() > 0:
        pytest.skip('CPU-container test: it spawns (execs) worker processes, which a process that may have initialised the GPU must not do')
    world = 2
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=90) for _ in range(world)]
    for p in procs:
        p.join(30)
        assert p.exitcode == 0
    return [r for r in res if r is not None][0]


def _expected(r, k):
    src = spread_chunk(r, k, k * T)
    prev = spread_start(r)[0] if k == 0 else spread_chunk(r, k - 1, (k - 1) * T)['obs'][T - 1][..., :4]
    return src, prev


@pytest.mark.timeout(240)
def test_two_ranks_fill_the_roots_per_agent_row_ring_rank_by_rank(root):
    ingested, ring = root['rows_ring']
    assert ingested == CHUNKS * 2 * T * B and len(ring) == CHUNKS * 2
    i = 0
    for k in range(CHUNKS):
        for r in range(2):
            src, _ = _expected(r, k)
            got = ring[i]
            want_next = torch.where(src['terminal'][:, :, None, None], src['final_obs'], src['obs']).reshape(T * B, N, -1)
            np.testing.assert_array_equal(got['next_obs'], want_next.numpy())
            np.testing.assert_array_equal(got['act'], src['act'].reshape(T * B, N).numpy().astype(np.uint8))
            # the trailer really travelled: the per-agent plane of (rank, chunk), not the block's rew_shared and not a broadcast
            np.testing.assert_array_equal(got['rew'], agent_rewards(r, k, N).reshape(T * B, N).numpy())
            assert got['rew'].shape == (T * B, N) and (got['rew'].max(1) != got['rew'].min(1)).all()
            assert got['done'].shape == (T * B, N) and not got['done'].any()
            i += 1


@pytest.mark.timeout(240)
def test_two_ranks_fill_the_roots_per_agent_state_ring_through_host_buffers(root):
    ingested, (obs, act, rew, nxt, done) = root['state_ring']
    n = T * B
    assert ingested == CHUNKS * 2 * n and rew.shape == (CHUNKS * 2 * n, N) and done.shape == rew.shape and not done.any()
    i = 0
    for k in range(CHUNKS):
        for r in range(2):
            src, _ = _expected(r, k)
            np.testing.assert_array_equal(rew[i * n:(i + 1) * n], agent_rewards(r, k, N).reshape(n, N).numpy())
            want_next = torch.where(src['terminal'][:, :, None, None], src['final_obs'], src['obs']).reshape(n, N, -1)
            np.testing.assert_array_equal(nxt[i * n:(i + 1) * n], want_next.numpy())
            i += 1


@pytest.mark.timeout(240)
def test_two_ranks_fill_the_roots_per_agent_two_head_ring(root):
    ingested, ring = root['ref']
    assert ingested == CHUNKS * 2 * T * B and len(ring) == CHUNKS * 2
    i = 0
    for k in range(CHUNKS):
        for r in range(2):
            src = ref_chunk(r, k, k * T)
            got = ring[i]
            np.testing.assert_array_equal(got['act'], src['act'].reshape(T * B, 2, 2).numpy().astype(np.uint8))
            np.testing.assert_array_equal(got['rew'], agent_rewards(r, k, 2).reshape(T * B, 2).numpy())
            want_next = torch.where(src['terminal'][:, :, None, None], src['final_obs'], src['obs']).reshape(T * B, 2, 21)
            np.testing.assert_array_equal(got['next_obs'], want_next.numpy())
            assert got['done'].shape == (T * B, 2) and not got['done'].any()
            i += 1
