#!/usr/bin/env python3
"""The learner's LSTMs with gradient -- nn.LSTM (MIOpen's RNN path) against FusedLSTM (pw_lstm_train_forward / pw_lstm_train_backward
for the recurrence, torch GEMMs for the rest), on the GPU (there is no fallback: without one this fails).

    python tools/lstm_train_bench.py [--out profiles/lstm_train.txt]

(a) forward + backward of Y.square().sum() through one LSTM over the agent axis, input [b, N, 64], b = 1024, both served shapes
    (1 x 64: the critics' lstm; 2 x 32: the actor's bilstm), N in {3, 6, 12, 24, 48}: stock nn.LSTM against the same module after
    fuse_lstm.  Device events around ITERS calls after warm-up, five repeats per path, the two paths alternating; launch counts
    from torch.profiler.  Every row prints "stock - fused" beside the spread (max - min) of stock's five repeats.
(b) wall time per optimize() of the example learner (examples/madr_learner.py Trainer, attention critic) at N = 6: unpatched,
    fused_lstm, and fused_lstm + accelerate_trainer(targets=True, optimizer=True); same method, "unpatched - path" beside the
    spread of the unpatched repeats.
Exit status 1 if at N = 6, for either shape, FusedLSTM is not faster than nn.LSTM by more than the spread of nn.LSTM's repeats.
A row of (a) with stock ahead by more than that spread is an N that multiagent_rl_amd.lstm.HANDED_BACK should name (FusedLSTM.forward
hands those lengths back to nn.LSTM.forward); the table marks such rows.
"""
import argparse
import copy
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'examples'))

import torch  # noqa: E402

from critic_bench import device_time_us, launches  # noqa: E402  (tools/ is sys.path[0] when run as a script)

B, REPEATS = 1024, 5


def make_paths(dirs, H, N):
    from multiagent_rl_amd import lstm as L
    torch.manual_seed(N)
    stock = torch.nn.LSTM(64, H, num_layers=1, batch_first=True, bidirectional=dirs == 2).cuda()
    fused = copy.deepcopy(stock)
    assert L.fuse_lstm(fused) == 1
    handed_back = N in L.HANDED_BACK[(dirs, H)]
    x = torch.randn(B, N, 64, device='cuda')

    def path(module):
        xg = x.clone().requires_grad_(True)

        def run():
            for p in module.parameters():
                p.grad = None
            xg.grad = None
            module(xg)[0].square().sum().backward()
        return run
    return path(stock), path(fused), handed_back


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
    names = ('unpatched', 'fused_lstm', 'fused_lstm + targets + optimizer')
    trainers = {}
    for name in names:
        torch.manual_seed(1)
        tr = madr_learner.Trainer(ActorNetwork(D, 5), CriticNetwork(D + 5, 1), memory, batch_size=B, fused_lstm=name != 'unpatched')
        if name == names[2]:
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
    base = res[names[0]]
    for name in names:
        v = res[name]
        gain = '' if name == names[0] else '   unpatched - this = %.3f | spread of unpatched %.3f' % (
            sum(base) / len(base) - sum(v) / len(v), max(base) - min(base))
        lines.append('  %-34s mean %.3f  min %.3f  max %.3f   [%s]%s' % (name, sum(v) / len(v), min(v), max(v),
                                                                       ' '.join('%.3f' % x for x in v), gain))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=100)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('lstm_train_bench: needs a GPU (no fallback)')
    lines = ['(a) one LSTM over the agent axis, forward + backward of Y.square().sum(), input [b, N, 64], b = %d: device-event us per call '
             '(%d calls per repeat, %d repeats, paths alternating)' % (B, args.iters, REPEATS),
             '%-7s %-4s %-34s %-34s %-8s %-30s %s' % ('shape', 'N', 'nn.LSTM  mean [min, max]', 'FusedLSTM  mean [min, max]', 'a / b',
                                                    'stock - fused | spread of stock', 'launches stock | fused')]
    ok = True
    for dirs, H in ((1, 64), (2, 32)):
        for N in (3, 6, 12, 24, 48):
            stock, fused, handed_back = make_paths(dirs, H, N)
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
                note = '   (handed back to nn.LSTM.forward)'
            elif -gain > spread:
                note = '   STOCK AHEAD: hand this N back (multiagent_rl_amd.lstm.HANDED_BACK)'
            lines.append('%d x %-3d %-4d %8.1f [%8.1f, %8.1f] %8s %8.1f [%8.1f, %8.1f] %8s %-8.2f %8.1f | %-19.1f %s | %s%s' % (
                dirs, H, N, ma, min(ta), max(ta), '', mb, min(tb), max(tb), '', ma / mb, gain, spread, launches(stock), launches(fused),
                note))
            if N == 6:
                met = gain > spread
                ok = ok and met
                lines.append('        condition at N = 6: stock - fused = %.1f us against the spread of stock\'s repeats %.1f us: %s' % (
                    gain, spread, 'met' if met else 'NOT met'))
    learner_times(lines, 30)
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
