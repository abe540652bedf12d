#!/usr/bin/env python3
"""The tail of the learner's update -- two gradient clips, two Adam steps, two soft updates -- stock PyTorch-ROCm against the HIP
kernels (pw_adam_step), on the GPU (there is no fallback: without one this fails).

    python tools/optimizer_bench.py [--out profiles/optimizer_tail.txt]    # the tail alone + the per-optimize() figures
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/optimizer_bench.py --kernel-only   # kernel time

(a) stock:  clip_grad_norm_(critic, 0.5); critic Adam.step(); clip_grad_norm_(actor, 0.5); actor Adam.step(); soft_update of both
            targets as ddpg_gumbel_fix.py:36-47 writes it (t.copy_(t * (1 - tau) + p * tau) per parameter) -- torch.optim.Adam
            with its defaults, the only way through the tail before pw_adam_step existed;
(a') the same with the soft update as examples/madr_learner.py writes it (pt.mul_(1 - tau).add_(ps, alpha=tau)): the tail of the
            learner whose optimize() is timed below, and the figure its share is taken from;
(b) fused:  FusedAdam(max_norm=0.5, targets=..., tau=...).step() for the critic and for the actor: two launches.
The networks are the N = 6 learner's (ActorNetwork(16, 5): 12 tensors, CriticNetwork(21): 8 tensors); the gradients are fixed random
tensors (the tail's cost does not depend on their values).  Device events around ITERS calls after warm-up, five repeats per path,
the two paths alternating.  Launch counts: kernels seen by torch.profiler in one call of each path.
Then the example learner (examples/madr_learner.py Trainer with the attention critic, b = 1024): wall ms per optimize() for four
settings -- unpatched, fused targets, fused optimiser, both -- five repeats each, alternating.
Exit status 1 if path (b) is not faster than path (a) by more than the spread (max - min) of (a)'s five repeats.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'examples'))

import torch  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, 'tools'))
from critic_bench import device_time_us, launches  # noqa: E402

B, N, D, A, REPEATS, TAU, LR = 1024, 6, 16, 5, 5, 1e-2, 1e-2


def make_paths():
    from multiagent_rl_amd.critic import CriticNetwork
    from multiagent_rl_amd.optim import FusedAdam
    from multiagent_rl_amd.policy import ActorNetwork

    def nets(seed):
        torch.manual_seed(seed)
        pair = [ActorNetwork(D, A).cuda(), CriticNetwork(D + A, 1).cuda()]
        for net in pair:
            for p in net.parameters():
                p.grad = torch.randn_like(p) * 0.05
        return pair
    (actor, critic), (t_actor, t_critic) = nets(1), nets(2)
    (f_actor, f_critic), (ft_actor, ft_critic) = nets(1), nets(2)
    (m_actor, m_critic), (mt_actor, mt_critic) = nets(1), nets(2)
    opt_a, opt_c = torch.optim.Adam(actor.parameters(), LR), torch.optim.Adam(critic.parameters(), LR)
    mopt_a, mopt_c = torch.optim.Adam(m_actor.parameters(), LR), torch.optim.Adam(m_critic.parameters(), LR)
    fopt_a = FusedAdam(f_actor.parameters(), LR, max_norm=0.5, targets=ft_actor.parameters(), tau=TAU)
    fopt_c = FusedAdam(f_critic.parameters(), LR, max_norm=0.5, targets=ft_critic.parameters(), tau=TAU)

    def soft(target, source):
        for tp, sp in zip(target.parameters(), source.parameters()):
            tp.data.copy_(tp.data * (1.0 - TAU) + sp.data * TAU)

    def stock():
        torch.nn.utils.clip_grad_norm_(critic.parameters(), 0.5)
        opt_c.step()
        torch.nn.utils.clip_grad_norm_(actor.parameters(), 0.5)
        opt_a.step()
        soft(t_actor, actor)
        soft(t_critic, critic)

    @torch.no_grad()
    def madr():
        torch.nn.utils.clip_grad_norm_(m_critic.parameters(), 0.5)
        mopt_c.step()
        torch.nn.utils.clip_grad_norm_(m_actor.parameters(), 0.5)
        mopt_a.step()
        for tgt, src in ((mt_actor, m_actor), (mt_critic, m_critic)):
            for pt, ps in zip(tgt.parameters(), src.parameters()):
                pt.mul_(1.0 - TAU).add_(ps, alpha=TAU)

    def fused():
        fopt_c.step()
        fopt_a.step()
    sizes = [(sum(1 for _ in n.parameters()), sum(p.numel() for p in n.parameters())) for n in (actor, critic)]
    return stock, madr, fused, sizes


def learner_times(lines, iters):
    """Wall time per optimize() of the example learner at N = 6: unpatched / fused targets / fused optimiser / both."""
    import madr_learner
    from multiagent_rl_amd import make_batched_env
    from multiagent_rl_amd.critic import CriticNetwork
    from multiagent_rl_amd.policy import ActorNetwork, FusedActor, accelerate_trainer
    from multiagent_rl_amd.replay_buffer import ReplayBuffer
    env = make_batched_env('simple_spread', 1024, auto_reset=True, max_episode_len=25, seed=1, n=N)
    env.reset()
    memory = ReplayBuffer(int(1e5), N, env.obs_dim, device_index=True)
    torch.manual_seed(0)
    FusedActor(ActorNetwork(env.obs_dim, A).cuda().eval(), seed=1).rollout(env, 50, out=False, memory=memory)
    settings = [('unpatched', False, False), ('targets', True, False), ('optimizer', False, True), ('targets + optimizer', True, True)]
    trainers = {}
    for name, targets, optimizer in settings:
        torch.manual_seed(1)
        tr = madr_learner.Trainer(ActorNetwork(env.obs_dim, A), CriticNetwork(env.obs_dim + A, 1), memory, batch_size=B,
                                  fused_optimizer=optimizer)
        if targets:
            accelerate_trainer(tr, targets=True)
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
    lines.append('examples/madr_learner.py Trainer, attention critic, simple_spread N = 6, b = %d: wall ms per optimize() '
                 '(%d calls per repeat, %d repeats, settings alternating)' % (B, iters, REPEATS))
    means = {}
    for name, _, _ in settings:
        v = res[name]
        means[name] = sum(v) / len(v)
        lines.append('  %-22s mean %.3f  min %.3f  max %.3f   [%s]' % (name, means[name], min(v), max(v), ' '.join('%.3f' % x for x in v)))
    return means


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--out', default=None)
    ap.add_argument('--kernel-only', action='store_true', help='200 fused tails and nothing else (for rocprofv3)')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('optimizer_bench: needs a GPU (no fallback)')
    stock, madr, fused, sizes = make_paths()
    if args.kernel_only:
        for _ in range(200):
            fused()
        torch.cuda.synchronize()
        return 0
    for _ in range(20):
        stock()
        madr()
        fused()
    torch.cuda.synchronize()
    ta, tm, tb = [], [], []
    for _ in range(REPEATS):
        ta.append(device_time_us(stock, args.iters))
        tm.append(device_time_us(madr, args.iters))
        tb.append(device_time_us(fused, args.iters))
    ma, mm, mb = sum(ta) / REPEATS, sum(tm) / REPEATS, sum(tb) / REPEATS
    lines = ['The tail of one update at N = 6 (actor %d tensors / %d elements, critic %d / %d): 2 clips + 2 Adam steps + 2 soft updates; '
             'device-event us per tail (%d tails per repeat, %d repeats, paths alternating)' % (*sizes[0], *sizes[1], args.iters, REPEATS),
             '  (a) stock PyTorch-ROCm   mean %8.1f  min %8.1f  max %8.1f   [%s]   launches %s' % (
                 ma, min(ta), max(ta), ' '.join('%.1f' % x for x in ta), launches(stock)),
             "  (a') madr_learner's form  mean %8.1f  min %8.1f  max %8.1f   [%s]   launches %s" % (
                 mm, min(tm), max(tm), ' '.join('%.1f' % x for x in tm), launches(madr)),
             '  (b) FusedAdam (HIP)      mean %8.1f  min %8.1f  max %8.1f   [%s]   launches %s' % (
                 mb, min(tb), max(tb), ' '.join('%.1f' % x for x in tb), launches(fused)),
             "  a / b = %.2f   a' / b = %.2f" % (ma / mb, mm / mb)]
    ok = ma - mb > max(ta) - min(ta)
    lines.append('condition: (a) - (b) = %.1f us against the spread of (a)\'s repeats %.1f us: %s' % (
        ma - mb, max(ta) - min(ta), 'met' if ok else 'NOT met'))
    means = learner_times(lines, 30)
    lines.append("  this learner's stock tail (a') is %.1f %% of its unpatched optimize(), %.1f %% of optimize() with fused targets "
                 '(device time of the tail over wall time of the update)' % (
                     100.0 * mm * 1e-3 / means['unpatched'], 100.0 * mm * 1e-3 / means['targets']))
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
