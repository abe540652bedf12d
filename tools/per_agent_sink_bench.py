#!/usr/bin/env python3
"""The per-agent ring sink of the one-launch rollouts (pw_rollout_sink with pw_replay_store.per_agent), on the GPU (no fallback).

    python tools/per_agent_sink_bench.py --parent _ab/head [--out profiles/per_agent_sink.txt]

The method of tools/head_train_bench.py: the paths alternate in one session, five repeats, mean / min / max, the difference held
against the spread (max - min) of the first path's repeats.  Configurations: C2 (simple_spread N = 6, B = 4096) and simple_tag 4 + 2 at
B = 8192, 100 steps per launch, episodes of 25 steps; wall ms per chunk over 200 chunks per repeat.

(a) What existed must not pay: BatchedRollout.collect_one_launch into a SHARED row ring and a shared STATE ring, the library of the tree
    under --parent (a checkout of the parent commit with its own libpworld.so) against this tree's.  Two libraries do not share a
    process, so every repeat is one child process per side, started in turn.
(b) The BiCNet chunk: collect_one_launch with a per-agent memory -- the two launches of before (the rollout with the statistics sink and
    all outputs, then ReplayBuffer.add_rollout; restated here, with its two sets of output buffers), the sink into the per-agent row ring
    and into the per-agent STATE ring with keep_outputs, and both sinks once more without outputs -- in one process, this tree's library.
"""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REPEATS, CHUNKS, T = 5, 200, 100
CONFIGS = {'C2 simple_spread N=6 B=4096': ('simple_spread', 4096), 'simple_tag 4+2 B=8192': ('simple_tag', 8192)}


def _env(scenario, B):
    from multiagent_rl_amd.env import BatchedParticleEnv
    if scenario == 'simple_tag':
        return BatchedParticleEnv('simple_tag', B, num_adversaries=4, num_good=2, max_episode_len=25, auto_reset=True, seed=1)
    return BatchedParticleEnv('simple_spread', B, num_agents=6, max_episode_len=25, auto_reset=True, seed=1)


def _rollout(scenario, B, state, per_agent):
    import torch
    from multiagent_rl_amd.policy import ActorNetwork, FusedActor
    from multiagent_rl_amd.replay_buffer import ReplayBuffer
    from multiagent_rl_amd.rollout import BatchedRollout
    torch.manual_seed(0)
    env = _env(scenario, B)
    kw = dict(per_agent=True) if per_agent else {}
    if state:
        kw['state_ring'] = dict(scenario=scenario, num_landmarks=env.num_landmarks,
                                num_adversaries=env.cfg.num_adversaries if scenario == 'simple_tag' else 0)
    mem = ReplayBuffer(int(1e6), env.n, env.obs_dim, **kw)
    return BatchedRollout(env, FusedActor(ActorNetwork(env.obs_dim, 5).cuda().eval(), seed=2), mem)


def _two_launches(ro, num_steps):
    """collect_one_launch with a per-agent memory as it ran until 0.1.21: the rollout writes every output, add_rollout reads them back."""
    stats = (ro.episode_return, ro.finished_return_sum, ro.finished_episodes)
    bufs = ro.__dict__.setdefault('_bench_bufs', {})
    obs0 = ro.__dict__.get('_bench_obs0', ro.obs)
    for _ in range(num_steps // T):
        flip = ro._bench_flip = 1 - getattr(ro, '_bench_flip', 0)
        out = bufs[flip] = ro.policy.rollout(ro.env, T, bufs.get(flip), memory=None, stats=stats)
        ro.memory.add_rollout(obs0.contiguous(), out)
        obs0 = out['obs'][T - 1]
    ro._bench_obs0 = obs0


def _ms_per_chunk(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / CHUNKS * 1e3


def child_shared():
    """One side of (a): {configuration / ring: ms per chunk}, one JSON line."""
    res = {}
    for name, (scenario, B) in CONFIGS.items():
        for state in (False, True):
            ro = _rollout(scenario, B, state, per_agent=False)
            ro.collect_one_launch(2 * T, chunk=T)
            res['%s, shared %s ring' % (name, 'STATE' if state else 'row')] = _ms_per_chunk(lambda: ro.collect_one_launch(CHUNKS * T, chunk=T))
            del ro
    print(json.dumps(res), flush=True)


def _table(lines, res, first, what):
    mean = lambda v: sum(v) / len(v)  # noqa: E731
    for name, v in res.items():
        lines.append('  %-44s mean %.4f  min %.4f  max %.4f   [%s]' % (name, mean(v), min(v), max(v), ' '.join('%.4f' % x for x in v)))
    spread = max(res[first]) - min(res[first])
    for name, v in res.items():
        if name == first:
            continue
        diff = mean(v) - mean(res[first])
        verdict = 'within the spread' if abs(diff) <= spread else ('SLOWER by more than the spread' if diff > 0 else 'faster by more than the spread')
        lines.append('  (%s) - (%s) = %+.4f ms per %s against the spread %.4f ms of the first path\'s repeats: %s'
                     % (name, first, diff, what, spread, verdict))
    lines.append('')


def shared_ab(parent, lines):
    sides = {'parent': os.path.abspath(parent), 'this tree': ROOT}
    res = {}
    for rep in range(REPEATS):
        for side, tree in sides.items():
            p = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', '--tree', tree], capture_output=True, text=True,
                               timeout=300)
            if p.returncode != 0:
                raise SystemExit('per_agent_sink_bench: the %s child failed (exit %d)\n%s' % (side, p.returncode, p.stderr[-2000:]))
            print('repeat %d, %s: done' % (rep + 1, side), file=sys.stderr, flush=True)
            for cfg, ms in json.loads(p.stdout.strip().splitlines()[-1]).items():
                res.setdefault(cfg, {}).setdefault(side, []).append(ms)
    for cfg, r in res.items():
        lines.append('(a) %s sink, %d steps per launch: wall ms per chunk (%d chunks per repeat, %d repeats, one process per side and '
                     'repeat, sides alternating)' % (cfg, T, CHUNKS, REPEATS))
        _table(lines, r, 'parent', 'chunk')


def bicnet_chunk(lines):
    import torch
    for cfg, (scenario, B) in CONFIGS.items():
        paths = {
            'two launches (rollout + add_rollout)': (_rollout(scenario, B, False, True), _two_launches),
            'sink, row ring, keep_outputs': (_rollout(scenario, B, False, True), lambda ro, n: ro.collect_one_launch(n, chunk=T, keep_outputs=True)),
            'sink, STATE ring, keep_outputs': (_rollout(scenario, B, True, True), lambda ro, n: ro.collect_one_launch(n, chunk=T, keep_outputs=True)),
            'sink, row ring, no outputs': (_rollout(scenario, B, False, True), lambda ro, n: ro.collect_one_launch(n, chunk=T)),
            'sink, STATE ring, no outputs': (_rollout(scenario, B, True, True), lambda ro, n: ro.collect_one_launch(n, chunk=T)),
        }
        res = {k: [] for k in paths}
        for ro, fn in paths.values():
            fn(ro, 2 * T)
        for _ in range(REPEATS):
            for name, (ro, fn) in paths.items():
                res[name].append(_ms_per_chunk(lambda: fn(ro, CHUNKS * T)))
        lines.append('(b) %s, per-agent memory, %d steps per chunk: wall ms per chunk (%d chunks per repeat, %d repeats, paths '
                     'alternating in one process)' % (cfg, T, CHUNKS, REPEATS))
        _table(lines, res, 'two launches (rollout + add_rollout)', 'chunk')
        del paths
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent', default=None, help='a checkout of the parent commit with its library built: part (a); left out, (b) alone')
    ap.add_argument('--out', default=None)
    ap.add_argument('--child', action='store_true', help=argparse.SUPPRESS)
    ap.add_argument('--tree', default=ROOT, help=argparse.SUPPRESS)
    args = ap.parse_args()
    sys.path.insert(0, args.tree)
    if args.child:
        return child_shared()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('per_agent_sink_bench: needs a GPU (no fallback)')
    lines = []
    if args.parent:
        shared_ab(args.parent, lines)
    bicnet_chunk(lines)
    text = '\n'.join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
