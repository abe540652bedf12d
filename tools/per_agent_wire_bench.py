#!/usr/bin/env python3
"""The learner rank's append of one wire block: the shared entry point (pw_replay_add_state_wire) beside the per-agent one
(pw_replay_add_state_wire_agents, 0.1.23), on the GPU (no fallback).

    python tools/per_agent_wire_bench.py --parent _ab/head [--out profiles/per_agent_wire.txt]

The method of tools/per_agent_sink_bench.py: the sides alternate in one session, five repeats, mean / min / max, the difference held
against the spread (max - min) of the first side's repeats.  Configurations: C2 (simple_spread N = 6, B = 4096) and simple_tag 4 + 2 at
B = 8192, T = 100 steps per block, episodes of 25 steps; for each, state block -> STATE ring and state block -> row ring.  One block is
filled by a real rollout chunk (FullTransitionGather with one rank: rollout into the block, finalize), then appended APPENDS times in a
row to a ring of 10^6 slots, the cursor moving on as in a run; wall microseconds per append over the batch.

Every repeat is one child process per side, started in turn (two libraries do not share a process): the tree under --parent (a checkout
of the parent commit with its own libpworld.so) measures its shared entry point, this tree measures the shared and the per-agent entry
point, alternating inside the child.  What must hold: this tree's shared append differs from the parent's by less than the spread of the
parent's repeats (tools/code_object.py --compare shows why: the kernels are the same code).  The per-agent append has no number to meet:
its time stands next to the bytes it moves.
"""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REPEATS, APPENDS, T = 5, 200, 100
CONFIGS = {'C2 simple_spread N=6 B=4096': ('simple_spread', 4096), 'simple_tag 4+2 B=8192': ('simple_tag', 8192)}


def _env(scenario, B):
    from multiagent_rl_amd.env import BatchedParticleEnv
    if scenario == 'simple_tag':
        return BatchedParticleEnv('simple_tag', B, num_adversaries=4, num_good=2, max_episode_len=25, auto_reset=True, seed=1)
    return BatchedParticleEnv('simple_spread', B, num_agents=6, max_episode_len=25, auto_reset=True, seed=1)


def _gather(scenario, B, ring, per_agent):
    """A one-rank gather whose slot 0 holds one real chunk's block (and trailer), appended once."""
    import torch
    from multiagent_rl_amd.dist import FullTransitionGather
    from multiagent_rl_amd.policy import ActorNetwork, FusedActor
    torch.manual_seed(0)
    env = _env(scenario, B)
    kw = dict(per_agent=True) if per_agent else {}
    g = FullTransitionGather(env, T, 0, 1, torch.device('cuda', 0), ring=ring, overlap_ingest=False, **kw)
    actor = FusedActor(ActorNetwork(env.obs_dim, 5).cuda().eval(), seed=2)
    env.reset()
    obs0 = env.observe()
    actor.rollout(env, T, g.outputs())
    g(obs0)
    g.finish()
    torch.cuda.synchronize()
    assert len(g.memory) == T * B
    return g


def _us_per_append(g):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(APPENDS):
        g._ingest(g.wire[0])
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / APPENDS * 1e6


def child(with_agents):
    """One side of one repeat: {configuration, ring, entry point: us per append}, one JSON line."""
    import torch
    res = {}
    for name, (scenario, B) in CONFIGS.items():
        for ring in ('state', 'rows'):
            sides = {'shared': _gather(scenario, B, ring, False)}
            if with_agents:
                sides['per-agent'] = _gather(scenario, B, ring, True)
            for g in sides.values():
                _us_per_append(g)                 # warm: the first launches, the ring's pages
            acc = {k: [] for k in sides}
            for _ in range(3):                    # the two entry points alternate inside the child as well
                for k, g in sides.items():
                    acc[k].append(_us_per_append(g))
            for k, v in acc.items():
                res['%s | %s | %s' % (name, 'STATE ring' if ring == 'state' else 'row ring', k)] = sorted(v)[1]      # the median of three
            g0 = sides['shared']
            res['%s | %s | bytes' % (name, 'STATE ring' if ring == 'state' else 'row ring')] = dict(
                N=g0.N, L=g0.L, D=g0.D, wire_shared=g0.bytes_per_env_step,
                wire_agents=sides['per-agent'].bytes_per_env_step if with_agents else None)
            del sides, g0
            torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)


def _ring_bytes(N, L, D, state, per_agent):
    """Bytes the append writes per transition: the two observation planes (a STATE ring: 16 B per agent each, and the landmarks), the
    action bytes, the reward / done words."""
    planes = 32 * N + 8 * L if state else 8 * N * D
    return planes + N + (8 * N if per_agent else 8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent', default=None, help='a checkout of the parent commit with its library built; left out: this tree alone')
    ap.add_argument('--out', default=None)
    ap.add_argument('--child', choices=['parent', 'this'], default=None, help=argparse.SUPPRESS)
    ap.add_argument('--tree', default=ROOT, help=argparse.SUPPRESS)
    args = ap.parse_args()
    sys.path.insert(0, args.tree)
    if args.child:
        return child(args.child == 'this')
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('per_agent_wire_bench: needs a GPU (no fallback)')
    sides = {'this tree': ('this', ROOT)}
    if args.parent:
        sides = {'parent': ('parent', os.path.abspath(args.parent)), 'this tree': ('this', ROOT)}
    res, info = {}, {}
    for rep in range(REPEATS):
        for side, (mode, tree) in sides.items():
            p = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', mode, '--tree', tree], capture_output=True, text=True,
                               timeout=300)
            if p.returncode != 0:
                raise SystemExit('per_agent_wire_bench: the %s child failed (exit %d)\n%s' % (side, p.returncode, p.stderr[-2000:]))
            print('repeat %d, %s: done' % (rep + 1, side), file=sys.stderr, flush=True)
            for key, v in json.loads(p.stdout.strip().splitlines()[-1]).items():
                cfg, ring, what = key.split(' | ')
                if what == 'bytes':
                    info.setdefault((cfg, ring), {}).update({k: x for k, x in v.items() if x is not None})
                else:
                    res.setdefault((cfg, ring), {}).setdefault('%s, %s entry point' % (side, what), []).append(v)
    mean = lambda v: sum(v) / len(v)  # noqa: E731
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    lines = ['append of one state block (T = %d) to a ring of 10^6 slots: wall us per append (%d appends per batch, the median of three '
             'batches per child, %d repeats = child processes per side, sides alternating)' % (T, APPENDS, REPEATS), '']
    for (cfg, ring), r in res.items():
        i = info[(cfg, ring)]
        B = CONFIGS[cfg][1]
        lines.append('%s, state block -> %s' % (cfg, ring))
        for name, v in r.items():
            pa = 'per-agent' in name
            nbytes = _ring_bytes(i['N'], i['L'], i['D'], ring == 'STATE ring', pa)
            lines.append('  %-38s median %8.2f  mean %8.2f  min %8.2f  max %8.2f  spread %6.2f   [%s]   writes %d B per transition '
                         '(%.1f MB per block: %.0f GB/s at the median), reads %.1f B per env-step off the wire block'
                         % (name, med(v), mean(v), min(v), max(v), max(v) - min(v), ' '.join('%.2f' % x for x in v), nbytes,
                            nbytes * T * B / 1e6, nbytes * T * B / med(v) / 1e3, i['wire_agents' if pa else 'wire_shared']))
        if 'parent, shared entry point' in r:
            a, b = r['parent, shared entry point'], r['this tree, shared entry point']
            spread, diff = max(a) - min(a), med(b) - med(a)
            lines.append('  shared entry point, this tree - parent = %+.2f us (medians) against the spread %.2f us of the parent\'s repeats: %s'
                         % (diff, spread, 'within the spread' if abs(diff) <= spread else ('SLOWER by more than the spread' if diff > 0
                                                                                          else 'faster by more than the spread')))
        if 'this tree, per-agent entry point' in r:
            a, b = r['this tree, shared entry point'], r['this tree, per-agent entry point']
            lines.append('  per-agent - shared (this tree) = %+.2f us (medians): %d more bytes written and %.1f more read per transition'
                         % (med(b) - med(a), 8 * i['N'] - 8, i['wire_agents'] - i['wire_shared']))
        lines.append('')
    lines.append('bytes per env-step on the wire (T = 100, episodes of 25: the per-chunk planes included): ' + '; '.join(
        '%s: shared %.1f, per-agent %.1f (17N + 5 = %d, 21N + 5 = %d)' % (cfg, i['wire_shared'], i.get('wire_agents', float('nan')),
                                                                         17 * i['N'] + 5, 21 * i['N'] + 5)
        for (cfg, ring), i in info.items() if ring == 'STATE ring'))
    text = '\n'.join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
