"""Worker of tests/test_gpu_per_agent_two_ranks.py: ONE rank of a world of two that share GPU 0, process group "gloo" -- the per-agent
form of tests/two_rank_gpu_worker.py.

The full gather runs with ``per_agent=True``: every block travels with its trailer plane (the per-agent rewards the rollout wrote behind
it) through pinned host buffers, and the root appends with the ``pw_replay_add_*wire_agents`` launches into a per-agent ring.  Every rank
also runs a twin of its shard whose rollout launch fills a local per-agent ROW ring through its own sink; the twins' rings go to rank 0
as CPU tensors, and rank 0 checks that its gathered ring holds, for exchange x and rank r, exactly rank r's chunk x at slots
[(x*world + r)*T*B, +T*B) -- bit for bit, ``rew`` / ``done`` [., N] included.  One JSON line per case on stdout (rank 0)."""
import json
import os
import sys

import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CHUNKS = 4
CASES = [
    # name, scenario, env kwargs, B, T, episode length, ring, wire
    ('spread_state_ring', 'simple_spread', dict(n=6), 96, 40, 25, 'state', 'auto'),
    ('spread_row_blocks', 'simple_spread', dict(n=6), 77, 26, 25, 'rows', 'rows'),
    ('tag_state_ring', 'simple_tag', dict(num_adversaries=4, num_good=2), 100, 40, 25, 'state', 'auto'),
    ('reference_two_head', 'simple_reference', dict(), 64, 40, 25, 'rows', 'auto'),
]


def run_case(rank, world, dev, name, scenario, kw, B, T, ep, ring, wire):
    from multiagent_rl_amd import make_batched_env
    from multiagent_rl_amd.dist import FullTransitionGather
    from multiagent_rl_amd.policy import ActorNetwork, FusedActor
    from multiagent_rl_amd.replay_buffer import ReplayBuffer
    torch.manual_seed(0)                                             # the same weights on every rank
    mk = lambda: make_batched_env(scenario, B, auto_reset=True, max_episode_len=ep, seed=11, env_id_base=rank * B, **kw)  # noqa: E731
    env_a, env_b = mk(), mk()
    N, D = env_a.n, env_a.obs_dim
    two = scenario == 'simple_reference'
    net = ActorNetwork(D, [5, 10] if two else 5).to(dev).eval()
    wire_actor, sink_actor = FusedActor(net, seed=3 + rank), FusedActor(net, seed=3 + rank)
    full = FullTransitionGather(env_a, T, rank, world, dev, capacity=CHUNKS * world * T * B, ring=ring, wire=wire, per_agent=True)
    assert full.transport == 'host' and full.per_agent, full.transport
    full.prime()
    want = ReplayBuffer(CHUNKS * T * B, N, D, per_agent=True, **(dict(act_heads=(5, 10)) if two else {}))
    env_a.reset()
    env_b.reset()
    obs0 = env_a.observe()
    for k in range(CHUNKS):
        out = full.outputs()
        wire_actor.rollout(env_a, T, out)
        full(obs0)
        obs0 = out['obs'][T - 1].clone()
        sink_actor.rollout(env_b, T, False, memory=want)
    full.finish()
    torch.cuda.synchronize()
    n = CHUNKS * T * B
    mine = [x.cpu().contiguous() for x in want.sample_index(list(range(n)))]
    assert tuple(mine[2].shape) == tuple(mine[4].shape) == (n, N)
    if rank:
        for x in mine:
            dist.send(x, 0)
        return None
    parts = [mine]
    for r in range(1, world):
        theirs = [torch.empty_like(x) for x in mine]
        for x in theirs:
            dist.recv(x, r)
        parts.append(theirs)
    mem = full.memory
    assert full.rows_ingested == world * n == len(mem), (full.rows_ingested, len(mem))
    assert mem.per_agent and tuple(mem.rew.shape) == tuple(mem.done.shape) == (world * n, N) and not mem.done.any()
    names = ('obs', 'act', 'rew', 'next_obs', 'done')
    for x in range(CHUNKS):
        for r in range(world):
            lo = (x * world + r) * T * B
            got = mem.sample_index(list(range(lo, lo + T * B)))
            for nm, g, w in zip(names, got, parts[r]):
                assert torch.equal(g.cpu(), w[x * T * B:(x + 1) * T * B]), (name, 'exchange', x, 'rank', r, nm)
    assert all(not torch.equal(parts[0][0], parts[r][0]) for r in range(1, world))        # the shards are different worlds
    per_agent_rewards = int(sum((p[2].max(1).values != p[2].min(1).values).sum() for p in parts))
    assert per_agent_rewards > 0                                     # a condition on the inputs: not a broadcast of the shared reward
    if ring == 'state':
        assert tuple(mem.obs.shape[1:]) == (N, 4) and mem.state_ring is not None
    return dict(case=name, world=world, transitions=world * n, bytes_per_env_step=round(full.bytes_per_env_step, 1),
                wire='ref' if full.ref_wire else 'state' if full.state_wire else 'rows', ring=ring,
                transitions_with_distinct_rewards=per_agent_rewards, ok=True)


def run_entry(argv):
    """``examples/train_batched.py`` as this rank (its ``main`` sets up the process group itself); rank 0 reports the ring its learner
    sampled from -- the one thing the script's own output does not show."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, 'examples'))
    import madr_learner
    import train_batched as entry
    seen = {}
    inner = madr_learner.Trainer.optimize

    def recording(self):
        seen['memory'] = self.memory
        return inner(self)
    madr_learner.Trainer.optimize = recording
    (name, cnt, st), = entry.main(argv)
    if int(os.environ['RANK']) == 0:
        mem = seen.get('memory')
        print(json.dumps(dict(entry=name, stats={k: v for k, v in st.items() if k != 'wall_s'}, learner=mem is not None,
                              per_agent=bool(getattr(mem, 'per_agent', False)), state_ring=getattr(mem, 'state_ring', None) is not None,
                              rew_shape=list(mem.rew.shape) if mem is not None else None, filled=len(mem) if mem is not None else 0)),
              flush=True)


def main():
    if sys.argv[1:2] == ['entry']:
        return run_entry(sys.argv[2:])
    rank, world = int(os.environ['RANK']), int(os.environ['WORLD_SIZE'])
    dist.init_process_group('gloo', rank=rank, world_size=world)
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    only = sys.argv[1:]
    try:
        for case in CASES:
            if only and case[0] not in only:
                continue
            res = run_case(rank, world, dev, *case)
            if rank == 0:
                print(json.dumps(res), flush=True)
            dist.barrier()
    finally:
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
