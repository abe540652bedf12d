#!/usr/bin/env python3
"""The output layers of the learner's networks on the HIP kernels (multiagent_rl_amd/heads.py) inside the graphed update, against the
graphed update with the stock output layers, on the GPU (there is no fallback: without one this fails).

    python tools/head_train_bench.py [--out profiles/head_train.txt]

(a) The method of tools/front_train_bench.py: wall ms per optimize() of the example learners (examples/madr_learner.py), b = 1024,
30 calls per repeat, five repeats, the paths alternating in one session.  Paths: every other switch + the graphed update (fused targets,
optimiser, LSTM, W_hh gradients, attention, sampling, front) -- the configuration before this switch existed; the same with
fused_heads.  Learners: Trainer with the attention critic at N = 3, 6 and 12 (rows of simple_spread's width, D = 6 N); once each the
two-head actor (simple_reference's dimensions: N = 2, D = 21, heads of 5 and 10), BiCNetTrainer and ModelTrainer at N = 6.  The rings
hold 4096 seeded random transitions (the update's cost does not depend on what the rows hold).  Under every table "(without - with the
heads)" beside the spread (max - min) of the first path's repeats, and whether it clears it; and the device kernels per update of both
paths, counted by torch.profiler in this same run (tools/critic_bench.py launches: one graph launch from the host, plus the eager refresh
of the exploration actor's snapshot, which the count includes).

(b) The family alone: forward + backward of head_projection against the stock expression (relu, one linear per head, and their
autograd) for the actor's shape (rows = 6144, one head of 5, ReLU, gradient to X and the parameters) and the pooled critics' (rows =
1024, one head of 1, no ReLU), eager, 200 calls per repeat, five repeats alternating; device kernels of one forward + backward of each."""
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
NAMES = ('every other switch + graph', 'every other switch + graph + heads')

LEARNERS = {   # name -> (Trainer class, actor, critic, ring kwargs, action type, D of N)
    'attention': ('Trainer', lambda pol, cr, D: pol.ActorNetwork(D, 5), lambda pol, cr, D: cr.CriticNetwork(D + 5, 1), {}, 'Discrete'),
    'two heads': ('Trainer', lambda pol, cr, D: pol.ActorNetwork(D, [5, 10]), lambda pol, cr, D: cr.CriticNetwork(D + 15, 1),
                  dict(act_heads=(5, 10)), 'MultiDiscrete'),
    'bicnet': ('BiCNetTrainer', lambda pol, cr, D: pol.ActorNetwork(D, 5), lambda pol, cr, D: cr.BiCNetCritic(D + 5, 1),
               dict(per_agent=True), 'Discrete'),
    'model': ('ModelTrainer', lambda pol, cr, D: pol.ModelActorNetwork(D, 5), lambda pol, cr, D: cr.ModelCriticNetwork(D + 5, 1), {},
              'Discrete'),
}


def _report(lines, res, what):
    mean = lambda v: sum(v) / len(v)  # noqa: E731
    stock, fused = (res[n] for n in res)
    for name, v in res.items():
        lines.append('  %-38s mean %.4f  min %.4f  max %.4f   [%s]' % (name, mean(v), min(v), max(v), ' '.join('%.4f' % x for x in v)))
    gain, spread = mean(stock) - mean(fused), max(stock) - min(stock)
    verdict = 'clears the spread' if gain > spread else ('stock is AHEAD by more than the spread' if -gain > spread else 'does NOT clear the spread')
    lines.append('  (without - with the heads) = %.4f ms per %s against the spread %.4f ms of the first path\'s repeats: %s' % (gain, what, spread, verdict))


def _filled_ring(ring_kw, N, D, n=4096):
    from multiagent_rl_amd.replay_buffer import ReplayBuffer
    rb = ReplayBuffer(8192, N, D, device_index='counter', index_seed=77, **ring_kw)
    g = torch.Generator().manual_seed(9)
    heads = ring_kw.get('act_heads', (5,))
    act = torch.stack([torch.randint(0, h, (n, N), generator=g) for h in heads], -1)
    rew = torch.randn((n, N) if ring_kw.get('per_agent') else (n,), generator=g)
    rb.add_batch(torch.randn(n, N, D, generator=g), act if len(heads) == 2 else act[..., 0], rew, torch.randn(n, N, D, generator=g),
                 done=(torch.rand(rew.shape, generator=g) < 0.1).float())
    return rb


def learner_times(kind, N, D, iters, lines):
    import madr_learner
    from multiagent_rl_amd import critic as cr, policy as pol
    cls_name, mk_actor, mk_critic, ring_kw, action_type = LEARNERS[kind]
    trainers = {}
    for name in NAMES:
        torch.manual_seed(1)
        trainers[name] = getattr(madr_learner, cls_name)(mk_actor(pol, cr, D), mk_critic(pol, cr, D), _filled_ring(ring_kw, N, D),
                                                         action_type=action_type, batch_size=B, fused_optimizer=True, fused_lstm=True,
                                                         fused_attention=True, graph_update=True, fused_sampling=True, fused_front=True,
                                                         fused_wgrad=True, fused_heads=name == NAMES[1])
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
    lines.append('examples/madr_learner.py %s, %s learner, N = %d (D = %d), b = %d: wall ms per optimize() '
                 '(%d calls per repeat, %d repeats, paths alternating)' % (cls_name, kind, N, D, B, iters, REPEATS))
    _report(lines, res, 'optimize()')
    counts = [launches(trainers[n].optimize) for n in NAMES]
    fewer = 'fewer with the heads' if all(c.isdigit() for c in counts) and int(counts[1]) < int(counts[0]) else 'NOT fewer with the heads'
    lines.append('  device kernels per update: without %s | with the heads %s: %s (one graph launch from the host; the count includes the '
                 'eager refresh of the exploration snapshot)' % (counts[0], counts[1], fewer))
    lines.append('')


def _device_kernels(fn):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return len([e for e in prof.events() if str(getattr(e, 'device_type', '')).endswith('CUDA')])


def family_alone(rows, widths, relu, iters, lines):
    import torch.nn as nn
    import torch.nn.functional as F
    from multiagent_rl_amd import heads
    torch.manual_seed(2)
    lins = [nn.Linear(64, n).cuda() for n in widths]
    x = torch.randn(rows, 64, device='cuda', requires_grad=True)
    dOuts = [torch.randn(rows, n, device='cuda') for n in widths]
    ws, bs = [lin.weight for lin in lins], [lin.bias for lin in lins]
    leaves = [x] + ws + bs

    def stock():
        a = F.relu(x) if relu else x
        torch.autograd.grad([F.linear(a, w, b) for w, b in zip(ws, bs)], leaves, dOuts)

    def fused():
        torch.autograd.grad(heads.head_projection(x, ws, bs, relu=relu), leaves, dOuts)
    paths = {'stock expression': stock, 'head_projection': fused}
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
    lines.append('the output layers alone, forward + backward, rows = %d, heads %r, relu %s: wall ms per call, eager '
                 '(%d calls per repeat, %d repeats, paths alternating)' % (rows, tuple(widths), bool(relu), iters, REPEATS))
    _report(lines, res, 'forward + backward')
    lines.append('  device kernels of one forward + backward: stock expression %d | head_projection %d' % (
        _device_kernels(stock), _device_kernels(fused)))
    lines.append('')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--agents', type=int, nargs='*', default=[3, 6, 12])
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('head_train_bench: needs a GPU (no fallback)')
    lines = []
    for N in args.agents:
        learner_times('attention', N, 6 * N, args.iters, lines)
    learner_times('two heads', 2, 21, args.iters, lines)
    learner_times('bicnet', 6, 36, args.iters, lines)
    learner_times('model', 6, 36, args.iters, lines)
    family_alone(6144, (5,), True, 200, lines)
    family_alone(1024, (1,), False, 200, lines)
    text = '\n'.join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
