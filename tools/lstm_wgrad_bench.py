#!/usr/bin/env python3
"""The W_hh gradients of the learner's LSTMs on the HIP kernels (multiagent_rl_amd.lstm.launch_wgrad) against the two sliced copies and a
GEMM per direction they replace, on the GPU (there is no fallback: without one this fails).

    python tools/lstm_wgrad_bench.py [--out profiles/lstm_wgrad.txt]

The method of tools/front_train_bench.py: both paths in one session, alternating, five repeats; the path without the switch is the
configuration before the switch existed.  Under every table "(without - with)" beside the spread (max - min) of the repeats without, and
whether it clears it.

(a) The backward of one LSTM alone (lstm_recurrence, gradient to G and every W_hh), eager, b = 1024, both shapes, N = 3, 6, 12, 24, 48,
200 calls per repeat; device kernels of one backward of each path (torch.profiler).  An N at which the GEMM path is ahead by more than
the spread belongs in lstm.WGRAD_HANDED_BACK.

(b) Wall ms per optimize() of the example learner (examples/madr_learner.py Trainer) with the attention critic on simple_spread,
b = 1024, every other switch on and the update graphed, 30 calls per repeat, at N = 3, 6 and 12, with and without fused_wgrad; device
kernels per update of both (tools/critic_bench.py launches: one graph launch from the host, plus the eager refresh of the exploration
actor's snapshot, which the count includes)."""
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
NAMES = ('every other switch + graph', 'every other switch + graph + wgrad')


def _report(lines, res, what):
    mean = lambda v: sum(v) / len(v)  # noqa: E731
    stock, fused = (res[n] for n in res)
    for name, v in res.items():
        lines.append('  %-38s mean %.4f  min %.4f  max %.4f   [%s]' % (name, mean(v), min(v), max(v), ' '.join('%.4f' % x for x in v)))
    gain, spread = mean(stock) - mean(fused), max(stock) - min(stock)
    verdict = 'clears the spread' if gain > spread else ('the GEMM path is AHEAD by more than the spread' if -gain > spread else 'does NOT clear the spread')
    lines.append('  (without - with) = %.4f ms per %s against the spread %.4f ms of the repeats without: %s' % (gain, what, spread, verdict))
    return -gain > spread


def _timed(paths, iters, warm):
    res = {k: [] for k in paths}
    for fn in paths.values():
        for _ in range(warm):
            fn()
    for _ in range(REPEATS):
        for name, fn in paths.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                fn()
            torch.cuda.synchronize()
            res[name].append((time.perf_counter() - t0) / iters * 1e3)
    return res


def _device_kernels(fn):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return len([e for e in prof.events() if str(getattr(e, 'device_type', '')).endswith('CUDA')])


def backward_alone(N, dirs, iters, lines):
    from multiagent_rl_amd import lstm as L
    H = 64 // dirs
    torch.manual_seed(2)
    G = torch.randn(B, N, dirs, 4 * H, device='cuda', requires_grad=True)
    ws = [(torch.randn(4 * H, H, device='cuda') / H ** 0.5).requires_grad_() for _ in range(dirs)]
    dY = torch.randn(B, N, dirs * H, device='cuda')
    leaves = [G] + ws
    held = {wgrad: L._Recurrence.apply(G, ws[0], ws[1] if dirs == 2 else None, False, wgrad)[0] for wgrad in (False, True)}
    paths = {'two copies + GEMM per direction': lambda: torch.autograd.grad(held[False], leaves, dY, retain_graph=True),
             'launch_wgrad': lambda: torch.autograd.grad(held[True], leaves, dY, retain_graph=True)}
    res = _timed(paths, iters, 20)
    lines.append('the backward of one LSTM alone (dG and every dW_hh), b = %d, N = %d, %d x %d hidden units: wall ms per call, eager '
                 '(%d calls per repeat, %d repeats, paths alternating)' % (B, N, dirs, H, iters, REPEATS))
    behind = _report(lines, res, 'backward')
    lines.append('  device kernels of one backward: GEMM path %d | launch_wgrad %d' % tuple(_device_kernels(fn) for fn in paths.values()))
    lines.append('')
    return behind


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
                                              fused_front=True, fused_wgrad=name == NAMES[1])
    res = _timed({n: t.optimize for n, t in trainers.items()}, iters, 10)   # the warm calls: beyond the three eager ones and the capture
    lines.append('examples/madr_learner.py Trainer, attention critic, simple_spread N = %d (D = %d), b = %d: wall ms per optimize() '
                 '(%d calls per repeat, %d repeats, paths alternating)' % (N, D, B, iters, REPEATS))
    _report(lines, res, 'optimize()')
    counts = [launches(trainers[n].optimize) for n in NAMES]
    fewer = 'fewer with the switch' if all(c.isdigit() for c in counts) and int(counts[1]) < int(counts[0]) else 'NOT fewer with the switch'
    lines.append('  device kernels per update: without %s | with fused_wgrad %s: %s (one graph launch from the host; the count includes the '
                 'eager refresh of the exploration snapshot)' % (counts[0], counts[1], fewer))
    lines.append('')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--agents', type=int, nargs='*', default=[3, 6, 12])
    ap.add_argument('--lengths', type=int, nargs='*', default=[3, 6, 12, 24, 48])
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('lstm_wgrad_bench: needs a GPU (no fallback)')
    lines, behind = [], {(1, 64): [], (2, 32): []}
    for dirs in (1, 2):
        for N in args.lengths:
            if backward_alone(N, dirs, 200, lines):
                behind[(dirs, 64 // dirs)].append(N)
    lines.append('lengths at which the GEMM path is ahead by more than its spread (lstm.WGRAD_HANDED_BACK): %r' % (
        {k: tuple(v) for k, v in behind.items()},))
    lines.append('')
    for N in args.agents:
        learner_times(N, args.iters, lines)
    text = '\n'.join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
