#!/usr/bin/env python3
"""The learner's update replayed as one captured graph (multiagent_rl_amd/graph.py) against the eager update, on the GPU (there is no
fallback: without one this fails).

    python tools/update_graph_bench.py [--out profiles/update_graph.txt]

The method of profiles/attention_train.txt (b): wall ms per optimize() of the example learner (examples/madr_learner.py Trainer) with the
attention critic on simple_spread, b = 1024, 30 calls per repeat, five repeats, the paths alternating in one session, at N = 6 and
also at N = 3 and N = 12.  Paths: unpatched; all four switches (fused_lstm + fused_attention + fused optimiser + fused targets); all
four + the graphed update.  Beside every row "unpatched - this"; under every table "(four switches - graph)" beside the spread
(max - min) of the four-switch repeats, and whether it clears it; and the device kernels per update of the last two paths, counted by
torch.profiler (the eager path issues each of them from the host; the graphed path issues one graph launch, plus the eager refresh of
the exploration actor's snapshot, which the count includes)."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'examples'))

import torch  # noqa: E402

from critic_bench import launches  # noqa: E402  (tools/ is sys.path[0] when run as a script)

B, REPEATS = 1024, 5
NAMES = ('unpatched', 'all four switches', 'all four switches + graph')


def learner_times(N, iters, lines):
    import madr_learner
    from multiagent_rl_amd import make_batched_env
    from multiagent_rl_amd.critic import CriticNetwork
    from multiagent_rl_amd.policy import ActorNetwork, FusedActor, accelerate_trainer
    from multiagent_rl_amd.replay_buffer import ReplayBuffer
    env = make_batched_env('simple_spread', 1024, auto_reset=True, max_episode_len=25, seed=1, n=N)
    env.reset()
    D = env.obs_dim
    trainers = {}
    for name in NAMES:
        # one ring per path, each filled by 50 steps of the same actor: the graphed path draws its batches from device cells ('counter' mode)
        memory = ReplayBuffer(int(1e5), N, D, device_index='counter' if name == NAMES[2] else True)
        torch.manual_seed(0)
        FusedActor(ActorNetwork(D, 5).cuda().eval(), seed=1).rollout(env, 50, out=False, memory=memory)
        torch.manual_seed(1)
        on = name != NAMES[0]
        tr = madr_learner.Trainer(ActorNetwork(D, 5), CriticNetwork(D + 5, 1), memory, batch_size=B, fused_optimizer=on, fused_lstm=on,
                                  fused_attention=on, graph_update=name == NAMES[2])
        if name == NAMES[1]:
            accelerate_trainer(tr, targets=True)
        trainers[name] = tr
    res = {k: [] for k in trainers}
    for tr in trainers.values():
        for _ in range(10):          # beyond the graphed path's three eager calls and its capture
            tr.optimize()
    for _ in range(REPEATS):
        for name, tr in trainers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                tr.optimize()
            torch.cuda.synchronize()
            res[name].append((time.perf_counter() - t0) / iters * 1e3)
    lines.append('examples/madr_learner.py Trainer, attention critic, simple_spread N = %d, b = %d: wall ms per optimize() '
                 '(%d calls per repeat, %d repeats, paths alternating)' % (N, B, iters, REPEATS))
    mean = lambda v: sum(v) / len(v)  # noqa: E731
    base, four, graph = (res[n] for n in NAMES)
    for name in NAMES:
        v = res[name]
        gain = '' if name == NAMES[0] else '   unpatched - this = %.3f | spread of unpatched %.3f' % (mean(base) - mean(v), max(base) - min(base))
        lines.append('  %-28s mean %.3f  min %.3f  max %.3f   [%s]%s' % (name, mean(v), min(v), max(v), ' '.join('%.3f' % x for x in v), gain))
    gain, spread = mean(four) - mean(graph), max(four) - min(four)
    lines.append('  (four switches - graph) = %.3f ms per optimize() against the spread %.3f ms of the four-switch repeats: %s' % (
        gain, spread, 'clears the spread' if gain > spread else 'does NOT clear the spread'))
    lines.append('  device kernels per update: all four switches %s | + graph %s (one graph launch from the host; the count includes the eager '
                 'refresh of the exploration snapshot)' % (launches(trainers[NAMES[1]].optimize), launches(trainers[NAMES[2]].optimize)))
    lines.append('')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--agents', type=int, nargs='*', default=[6, 3, 12])
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('update_graph_bench: needs a GPU (no fallback)')
    lines = []
    for N in args.agents:
        learner_times(N, args.iters, lines)
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)
    return 0


if __name__ == '__main__':
    sys.exit(main())
