#!/usr/bin/env python3
"""The learner's Gumbel-softmax samples on the HIP kernels (multiagent_rl_amd/sampling.py) inside the graphed update, against the graphed
update with the stock F.gumbel_softmax, on the GPU (there is no fallback: without one this fails).

    python tools/sampling_bench.py [--out profiles/sampling_train.txt]

The method of tools/update_graph_bench.py: wall ms per optimize() of the example learner (examples/madr_learner.py Trainer) with the
attention critic on simple_spread, b = 1024, 30 calls per repeat, five repeats, the paths alternating in one session, at N = 6 and also
at N = 3 and N = 12.  Paths: all four switches + the graphed update; the same with fused_sampling.  Under every table "(graph - graph with
sampling)" beside the spread (max - min) of the first path's repeats, and whether it clears it; and the device kernels per update of both
paths, counted by torch.profiler in this same run (tools/critic_bench.py launches: one graph launch from the host, plus the eager refresh
of the exploration actor's snapshot, which the count includes).  The kernel counts are the criterion (fewer with sampling at every N);
the time is reported, and a speed-up is stated only where it clears the spread.

Below the tables: the measured maximum errors of the kernels against their float64 references at the shapes of tests/test_gpu_sampling.py
(the same figures that file asserts bounds on)."""
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
NAMES = ('all four switches + graph', 'all four switches + graph + sampling')


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
                                              fused_lstm=True, fused_attention=True, graph_update=True, fused_sampling=name == NAMES[1])
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
    lines.append('examples/madr_learner.py Trainer, attention critic, simple_spread N = %d, b = %d: wall ms per optimize() '
                 '(%d calls per repeat, %d repeats, paths alternating)' % (N, B, iters, REPEATS))
    mean = lambda v: sum(v) / len(v)  # noqa: E731
    stock, fused = (res[n] for n in NAMES)
    for name in NAMES:
        v = res[name]
        lines.append('  %-38s mean %.3f  min %.3f  max %.3f   [%s]' % (name, mean(v), min(v), max(v), ' '.join('%.3f' % x for x in v)))
    gain, spread = mean(stock) - mean(fused), max(stock) - min(stock)
    lines.append('  (graph - graph with sampling) = %.3f ms per optimize() against the spread %.3f ms of the first path\'s repeats: %s' % (
        gain, spread, 'clears the spread' if gain > spread else 'does NOT clear the spread'))
    counts = [launches(trainers[n].optimize) for n in NAMES]
    fewer = 'fewer with sampling' if all(c.isdigit() for c in counts) and int(counts[1]) < int(counts[0]) else 'NOT fewer with sampling'
    lines.append('  device kernels per update: + graph %s | + graph + sampling %s: %s (one graph launch from the host; the count includes the '
                 'eager refresh of the exploration snapshot)' % (counts[0], counts[1], fewer))
    lines.append('')


def kernel_errors(lines):
    """The figures tests/test_gpu_sampling.py bounds, measured: maxima over rows {1, 257, 6144}, n {1, 3, 4, 5, 10, 16}, tau {1, 0.5}."""
    import numpy as np
    from multiagent_rl_amd import sampling
    from oracle import actor_oracle as ao
    worst = dict(noise=0.0, soft_rel=0.0, formula=0.0, stock=0.0, left_out=0.0)
    mismatches = 0
    for rows in (1, 257, 6144):
        for n in (1, 3, 4, 5, 10, 16):
            x = 2 * torch.randn(rows, n, generator=torch.Generator().manual_seed(1000 * n + rows))
            dY = torch.randn(rows, n, generator=torch.Generator().manual_seed(rows + n)).cuda()
            for seed, step in ((7, 0), (7, 16), (2 ** 33 + 5, 2 ** 32 + 3)):
                want_noise = ao.gumbel_noise(seed, step, np.arange(rows), n)
                act, margin = ao.predict(x.double().numpy(), seed, step, np.arange(rows), (n,))
                for tau in (1.0, 0.5):
                    y, soft, idx, noise = sampling.launch_forward(x.cuda(), tau, True, seed, step, None, True, want_idx=True, want_noise=True)
                    worst['noise'] = max(worst['noise'], float(np.abs(noise.double().cpu().numpy() - want_noise).max()))
                    ok = margin[:, 0] > 1e-4
                    worst['left_out'] = max(worst['left_out'], 1.0 - float(ok.mean()))
                    mismatches += int((ok & (idx.cpu().numpy() != act[:, 0])).sum())
                    v = (x.cuda().double() - noise.double()) / tau
                    want = torch.softmax(v, -1)
                    err = (soft.double() - want).abs()
                    worst['soft_rel'] = max(worst['soft_rel'], float(((err - 1e-7).clamp_min(0) / want).max()))
                    got = sampling.launch_backward(dY, soft, tau).double()
                    scale = float(dY.abs().max()) / tau
                    d, s = dY.double(), soft.double()
                    worst['formula'] = max(worst['formula'], float((got - s * (d - (d * s).sum(-1, keepdim=True)) / tau).abs().max()) / scale)
                    xs = x.cuda().double().requires_grad_()
                    y_soft = ((xs - noise.double()) / tau).softmax(-1)
                    y_hard = torch.zeros_like(xs).scatter_(-1, y_soft.max(-1, keepdim=True)[1], 1.0)
                    ((y_hard - y_soft.detach() + y_soft) * d).sum().backward()
                    worst['stock'] = max(worst['stock'], float((got - xs.grad).abs().max()) / scale)
    lines.append('pw_gumbel_st_forward / pw_gumbel_st_backward against float64, maxima over rows {1, 257, 6144} x n {1, 3, 4, 5, 10, 16} x three '
                 '(seed, step) x tau {1, 0.5}:')
    lines.append('  |noise - oracle| %.3e (bound 1e-4); sampled index: %d mismatches at float64 margin > 1e-4, at most %.4f %% of the rows left out '
                 '(bound 0.1 %%)' % (worst['noise'], mismatches, 100 * worst['left_out']))
    lines.append('  soft: largest (|err| - 1e-7) / softmax %.3e (bound 5e-5)' % worst['soft_rel'])
    lines.append('  dLogits: against the float64 formula %.3e max|dY| / tau (bound 5e-6); against float64 autograd of the stock expression %.3e '
                 'max|dY| / tau (bound 2e-4)' % (worst['formula'], worst['stock']))
    lines.append('')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--agents', type=int, nargs='*', default=[6, 3, 12])
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('sampling_bench: needs a GPU (no fallback)')
    lines = []
    for N in args.agents:
        learner_times(N, args.iters, lines)
    kernel_errors(lines)
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)
    return 0


if __name__ == '__main__':
    sys.exit(main())
