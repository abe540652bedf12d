#!/usr/bin/env python3
"""The attention block of the learner's critic with gradient -- the stock expression of critic.py (bmm, softmax, bmm, relu under autograd)
against attention_pool (pw_attention_pool_forward / pw_attention_pool_backward), on the GPU (there is no fallback: without one this
fails).

    python tools/attention_bench.py [--out profiles/attention_train.txt]

(a) forward + backward of out.square().sum() through the block on Y [b, N, 64], b = 1024, N in {3, 6, 12, 24, 48}.  Device events
    around ITERS calls after warm-up, five repeats per path, the two paths alternating; launch counts from torch.profiler.  Every row
    prints "stock - fused" beside the spread (max - min) of stock's five repeats.
(b) wall time per optimize() of the example learner (examples/madr_learner.py Trainer, attention critic) at N = 6: unpatched, the best
    of the other switches (fused_lstm + accelerate_trainer(targets=True, optimizer=True)), and the same with fused_attention; same
    method, "unpatched - path" beside the spread of the unpatched repeats, and "best without - with attention" beside the spread of
    the former.
A row of (a) with stock ahead by more than that spread is an N that multiagent_rl_amd.attention.HANDED_BACK should name (a fused critic
hands those lengths back to the stock expression); the table marks such rows.  Exit status 1 if there is such a row that
HANDED_BACK does not name.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'examples'))

import torch  # noqa: E402

from critic_bench import device_time_us, launches  # noqa: E402  (tools/ is sys.path[0] when run as a script)

B, REPEATS = 1024, 5


def make_paths(N):
    from multiagent_rl_amd import attention as A
    torch.manual_seed(N)
    Y = torch.tanh(torch.randn(B, N, 64, device='cuda'))   # the size of an LSTM's output

    def path(fn):
        Yg = Y.clone().requires_grad_(True)

        def run():
            Yg.grad = None
            fn(Yg, True).square().sum().backward()
        return run
    return path(A.stock_attention), path(A.attention_pool), N in A.HANDED_BACK


def learner_times(lines, iters):
    import madr_learner
    from multiagent_rl_amd import make_batched_env
    from multiagent_rl_amd.critic import CriticNetwork
    from multiagent_rl_amd.policy import ActorNetwork, FusedActor, accelerate_trainer
    from multiagent_rl_amd.replay_buffer import ReplayBuffer
    N = 6
    env = make_batched_env('simple_spread', 1024, auto_reset=True, max_episode_len=25, seed=1, n=N)
    env.reset()
    D = env.obs_dim
    memory = ReplayBuffer(int(1e5), N, D, device_index=True)
    torch.manual_seed(0)
    FusedActor(ActorNetwork(D, 5).cuda().eval(), seed=1).rollout(env, 50, out=False, memory=memory)
    names = ('unpatched', 'fused_lstm + targets + optimizer', 'fused_lstm + targets + optimizer + fused_attention')
    trainers = {}
    for name in names:
        torch.manual_seed(1)
        tr = madr_learner.Trainer(ActorNetwork(D, 5), CriticNetwork(D + 5, 1), memory, batch_size=B, fused_lstm=name != names[0],
                                  fused_attention=name == names[2])
        if name != names[0]:
            accelerate_trainer(tr, targets=True, optimizer=True)
        trainers[name] = tr
    res = {k: [] for k in trainers}
    for tr in trainers.values():
        for _ in range(10):
            tr.optimize()
    for _ in range(REPEATS):
        for name, tr in trainers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                tr.optimize()
            torch.cuda.synchronize()
            res[name].append((time.perf_counter() - t0) / iters * 1e3)
    lines.append('')
    lines.append('(b) examples/madr_learner.py Trainer, attention critic, simple_spread N = 6, b = %d: wall ms per optimize() '
                 '(%d calls per repeat, %d repeats, paths alternating)' % (B, iters, REPEATS))
    mean = lambda v: sum(v) / len(v)  # noqa: E731
    base, best = res[names[0]], res[names[1]]
    for name in names:
        v = res[name]
        gain = '' if name == names[0] else '   unpatched - this = %.3f | spread of unpatched %.3f' % (mean(base) - mean(v), max(base) - min(base))
        lines.append('  %-52s mean %.3f  min %.3f  max %.3f   [%s]%s' % (name, mean(v), min(v), max(v), ' '.join('%.3f' % x for x in v), gain))
    gain, spread = mean(best) - mean(res[names[2]]), max(best) - min(best)
    lines.append('  fused_attention on top of the other switches: %.3f ms per optimize() against the spread %.3f ms of the repeats without it: %s' % (
        gain, spread, 'clears the spread' if gain > spread else 'does NOT clear the spread'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=100)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('attention_bench: needs a GPU (no fallback)')
    lines = ['(a) the attention block, forward + backward of out.square().sum(), Y [b, N, 64], b = %d: device-event us per call '
             '(%d calls per repeat, %d repeats, paths alternating)' % (B, args.iters, REPEATS),
             '%-4s %-34s %-34s %-8s %-30s %s' % ('N', 'stock  mean [min, max]', 'attention_pool  mean [min, max]', 'a / b',
                                                'stock - fused | spread of stock', 'launches stock | fused')]
    ok = True
    for N in (3, 6, 12, 24, 48):
        stock, fused, handed_back = make_paths(N)
        for _ in range(20):
            stock()
            fused()
        torch.cuda.synchronize()
        ta, tb = [], []
        for _ in range(REPEATS):
            ta.append(device_time_us(stock, args.iters))
            tb.append(device_time_us(fused, args.iters))
        ma, mb = sum(ta) / REPEATS, sum(tb) / REPEATS
        gain, spread = ma - mb, max(ta) - min(ta)
        note = ''
        if handed_back:
            note = '   (a fused critic hands this N back to the stock expression)'
        elif -gain > spread:
            note = '   STOCK AHEAD: hand this N back (multiagent_rl_amd.attention.HANDED_BACK)'
            ok = False
        lines.append('%-4d %8.1f [%8.1f, %8.1f] %8s %8.1f [%8.1f, %8.1f] %8s %-8.2f %8.1f | %-19.1f %s | %s%s' % (
            N, ma, min(ta), max(ta), '', mb, min(tb), max(tb), '', ma / mb, gain, spread, launches(stock), launches(fused), note))
    learner_times(lines, 30)
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
