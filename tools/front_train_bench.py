#!/usr/bin/env python3
"""The dense front of the learner's networks on the HIP kernels (multiagent_rl_amd/dense.py) inside the graphed update, against the
graphed update with the stock front, on the GPU (there is no fallback: without one this fails).

    python tools/front_train_bench.py [--out profiles/front_train.txt]

(a) The method of tools/sampling_bench.py: wall ms per optimize() of the example learner (examples/madr_learner.py Trainer) with the
attention critic on simple_spread, b = 1024, 30 calls per repeat, five repeats, the paths alternating in one session, at N = 3, 6 and
12.  Paths: every other switch + the graphed update (fused targets, optimiser, LSTM, attention, sampling); the same with fused_front.
Under every table "(without - with the front)" beside the spread (max - min) of the first path's repeats, and whether it clears it; and
the device kernels per update of both paths, counted by torch.profiler in this same run (tools/critic_bench.py launches: one graph launch
from the host, plus the eager refresh of the exploration actor's snapshot, which the count includes).

(b) The front alone: forward + backward of front_projection against the stock expression (the cat, dense1, the ReLU, the weight and bias
concatenations, the second linear, and their autograd) at rows = 6144, d0 = 16 + d1 = 5 for the critics' LSTM shape (1 x 64, gradient to
the parameters and the action part) and d0 = 16 for the actor's (2 x 32, gradient to the parameters), eager, 200 calls per repeat, five
repeats alternating; device kernels of one forward + backward of each."""
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
NAMES = ('every other switch + graph', 'every other switch + graph + front')


def _report(lines, res, what):
    mean = lambda v: sum(v) / len(v)  # noqa: E731
    stock, fused = (res[n] for n in res)
    for name, v in res.items():
        lines.append('  %-38s mean %.4f  min %.4f  max %.4f   [%s]' % (name, mean(v), min(v), max(v), ' '.join('%.4f' % x for x in v)))
    gain, spread = mean(stock) - mean(fused), max(stock) - min(stock)
    verdict = 'clears the spread' if gain > spread else ('stock is AHEAD by more than the spread' if -gain > spread else 'does NOT clear the spread')
    lines.append('  (without - with the front) = %.4f ms per %s against the spread %.4f ms of the first path\'s repeats: %s' % (gain, what, spread, verdict))


def learner_times(N, iters, lines):
    import madr_learner
    from multiagent_rl_amd import make_batched_env
    from multiagent_rl_amd.critic import CriticNetwork
    from multiagent_rl_amd.policy import ActorNetwork, FusedActor
    from multiagent_rl_amd.replay_buffer import ReplayBuffer
    env = make_batched_env('simple_spread', 1024, auto_reset=True, max_episode_len=25, seed=1, n=N)
    env.reset()
    D = env.obs_dim
    trainers = {}
    for name in NAMES:
        memory = ReplayBuffer(int(1e5), N, D, device_index='counter')   # one ring per path, each filled by 50 steps of the same actor
        torch.manual_seed(0)
        FusedActor(ActorNetwork(D, 5).cuda().eval(), seed=1).rollout(env, 50, out=False, memory=memory)
        torch.manual_seed(1)
        trainers[name] = madr_learner.Trainer(ActorNetwork(D, 5), CriticNetwork(D + 5, 1), memory, batch_size=B, fused_optimizer=True,
                                              fused_lstm=True, fused_attention=True, graph_update=True, fused_sampling=True,
                                              fused_front=name == NAMES[1])
    res = {k: [] for k in trainers}
    for tr in trainers.values():
        for _ in range(10):          # beyond the three eager calls and the capture
            tr.optimize()
    for _ in range(REPEATS):
        for name, tr in trainers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                tr.optimize()
            torch.cuda.synchronize()
            res[name].append((time.perf_counter() - t0) / iters * 1e3)
    lines.append('examples/madr_learner.py Trainer, attention critic, simple_spread N = %d (D = %d), b = %d: wall ms per optimize() '
                 '(%d calls per repeat, %d repeats, paths alternating)' % (N, D, B, iters, REPEATS))
    _report(lines, res, 'optimize()')
    counts = [launches(trainers[n].optimize) for n in NAMES]
    fewer = 'fewer with the front' if all(c.isdigit() for c in counts) and int(counts[1]) < int(counts[0]) else 'NOT fewer with the front'
    lines.append('  device kernels per update: without %s | with the front %s: %s (one graph launch from the host; the count includes the '
                 'eager refresh of the exploration snapshot)' % (counts[0], counts[1], fewer))
    lines.append('')


def _device_kernels(fn):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return len([e for e in prof.events() if str(getattr(e, 'device_type', '')).endswith('CUDA')])


def front_alone(rows, d0, d1, dirs, iters, lines):
    import torch.nn as nn
    import torch.nn.functional as F
    from multiagent_rl_amd import dense
    torch.manual_seed(2)
    lin, lstm = nn.Linear(d0 + d1, 64).cuda(), nn.LSTM(64, 64 // dirs, batch_first=True, bidirectional=dirs == 2).cuda()
    w_ih, b_ih, b_hh = dense._lstm_params(lstm)
    x0 = torch.randn(rows, d0, device='cuda')
    x1 = F.one_hot(torch.randint(0, d1, (rows,), device='cuda'), d1).float().requires_grad_() if d1 else None
    dG = torch.randn(rows, 256, device='cuda')
    params = [lin.weight, lin.bias] + w_ih + b_ih + b_hh
    leaves = params + ([x1] if d1 else [])

    def stock():
        hid = F.relu(lin(x0 if x1 is None else torch.cat([x0, x1], dim=-1)))
        if dirs == 2:
            w, b = torch.cat(w_ih, dim=0), torch.cat([b_ih[0] + b_hh[0], b_ih[1] + b_hh[1]], dim=0)
        else:
            w, b = w_ih[0], b_ih[0] + b_hh[0]
        torch.autograd.grad(F.linear(hid, w, b), leaves, dG)

    def fused():
        torch.autograd.grad(dense.front_projection(x0, x1, lin.weight, lin.bias, w_ih, b_ih, b_hh), leaves, dG)
    paths = {'stock expression': stock, 'front_projection': fused}
    res = {k: [] for k in paths}
    for fn in paths.values():
        for _ in range(20):
            fn()
    for _ in range(REPEATS):
        for name, fn in paths.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                fn()
            torch.cuda.synchronize()
            res[name].append((time.perf_counter() - t0) / iters * 1e3)
    lines.append('the front alone, forward + backward, rows = %d, d0 = %d, d1 = %d, %d x %d hidden units: wall ms per call, eager '
                 '(%d calls per repeat, %d repeats, paths alternating)' % (rows, d0, d1, dirs, 64 // dirs, iters, REPEATS))
    _report(lines, res, 'forward + backward')
    lines.append('  device kernels of one forward + backward: stock expression %d | front_projection %d' % (
        _device_kernels(stock), _device_kernels(fused)))
    lines.append('')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--agents', type=int, nargs='*', default=[3, 6, 12])
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('front_train_bench: needs a GPU (no fallback)')
    lines = []
    for N in args.agents:
        learner_times(N, args.iters, lines)
    front_alone(6144, 16, 5, 1, 200, lines)
    front_alone(6144, 16, 0, 2, 200, lines)
    text = '\n'.join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
