#!/usr/bin/env python3
"""The learner's no-gradient half -- target actor, Gumbel one-hot, target critic, TD target -- stock PyTorch-ROCm against the HIP
kernels, on the GPU (there is no fallback: without one this fails).

    python tools/critic_bench.py [--out profiles/critic_td_target.txt]     # the table + the per-optimize() figures
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/critic_bench.py --kernel-only   # kernel time (N = 6)

(a) stock:  logits1 = target_actor(s1); a1 = hard Gumbel one-hot; q = target_critic(s1, a1); y = r + GAMMA * q * (1 - d), under
            no_grad -- the only way to y before pw_critic_forward existed;
(b) fused:  FusedActor.logits (pw_actor_fused) + the same sampling + FusedCritic.td_target (pw_critic_forward with the epilogue).
b = 1024 (the reference's batch), simple_spread's local rows D = 4 + 2 N, N in {3, 6, 12, 24, 48}; device events around ITERS
calls after warm-up, five repeats per path, the two paths alternating.  The one-launch actor serves rows up to 104 numbers, so
every row of the table, N = 48 (D = 100) included, runs FusedActor.logits for the target actor.
Launch counts: kernels seen by torch.profiler in one call of each path.
    python tools/critic_bench.py --wide [--out profiles/actor_wide_rows.txt]   # N = 48 alone: (a), (b) and the mix that served
        N = 48 before the actor took rows longer than 64 numbers (stock target actor + pw_critic_forward), then the actor alone
        (stock ActorNetwork forward against FusedActor.logits); exit status 1 if the mix is not slower than (b) by more than the
        spread of the mix's repeats.
    python tools/critic_bench.py --bicnet [--out profiles/critic_steps_td_target.txt]   # the BiCNet baseline: per-step critic
        (BiCNetCritic, q and y on [b, N], per-agent r and d) at N in {3, 6, 12, 24, 48, 64}, D = min(4 + 2 N, 104): (a) stock against (b)
        pw_actor_fused + sampling + pw_critic_forward_steps, "stock - fused" beside the spread of stock's repeats; then, at N = 48 and 64,
        FusedCritic.q alone on the per-step kernel (16 rows per workgroup) beside the attention kernel (8 rows), at b = 1024 and b = 8192.  A record,
        not a gate.
    python tools/critic_bench.py --model [--out profiles/critic_model_td_target.txt]   # the model-learning variant: target
        ModelActorNetwork (the first of its pair), sampling, target ModelCriticNetwork (the first of its pair), y, at N in {3, 6, 12, 24}:
        (a) stock against (b) pw_actor_fused + sampling + pw_critic_forward_model (no reward head in that launch), "stock - fused"
        beside the spread of stock's repeats; then one optimize() of examples/madr_learner.py's ModelTrainer at N = 6, unpatched against
        all four switches.  A record, not a gate.
Then the example learner (examples/madr_learner.py Trainer with the attention critic) at N = 6: wall time per optimize() with and
without accelerate_trainer(targets=True), five repeats each, alternating.
Exit status 1 if at N = 6 path (b) is not faster than path (a) by more than the spread (max - min) of (a)'s five repeats.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'examples'))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

GAMMA, B, REPEATS = 0.95, 1024, 5


def make_paths(N, D, bicnet=False):
    from multiagent_rl_amd.critic import BiCNetCritic, CriticNetwork, FusedCritic
    from multiagent_rl_amd.policy import ActorNetwork, FusedActor
    torch.manual_seed(N)
    actor, critic = ActorNetwork(D, 5).cuda().eval(), (BiCNetCritic if bicnet else CriticNetwork)(D + 5, 1).cuda().eval()
    s1 = torch.randn(B, N, D, device='cuda')
    rd = (B, N) if bicnet else (B,)       # the BiCNet tuple: per-agent reward and done
    r, d = torch.randn(rd, device='cuda'), (torch.rand(rd, device='cuda') < 0.1).float()
    fused_actor = FusedActor(actor)
    fc = FusedCritic(critic)

    def sample(logits):
        return F.gumbel_softmax(logits.reshape(B * N, -1), hard=True).reshape(B, N, -1)

    @torch.no_grad()
    def stock():
        q = torch.squeeze(critic(s1, sample(actor(s1))))
        return r + GAMMA * q * (1. - d)

    @torch.no_grad()
    def fused():
        return fc.td_target(s1, sample(fused_actor.logits(s1)), r, d, GAMMA)

    @torch.no_grad()
    def mix():       # stock target actor + the fused critic
        return fc.td_target(s1, sample(actor(s1)), r, d, GAMMA)

    @torch.no_grad()
    def actor_stock():
        return actor(s1)

    @torch.no_grad()
    def actor_fused():
        return fused_actor.logits(s1)
    return stock, fused, dict(mix=mix, actor_stock=actor_stock, actor_fused=actor_fused)


def device_time_us(fn, iters):
    beg, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    beg.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return beg.elapsed_time(end) * 1e3 / iters


def launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, 'device_type', '')).endswith('CUDA'))
        return str(n) if n else 'n/a'
    except Exception as exc:   # the count is a by-product: the timings do not depend on the profiler
        return 'n/a (%s)' % type(exc).__name__


def wide_rows(args):
    """N = 48 (D = 100): the TD target on three paths and the actor alone, same method as the table."""
    N, D = 48, 100
    stock, fused, more = make_paths(N, D)
    paths = [('(a) stock PyTorch-ROCm', stock), ('(m) stock target actor + pw_critic_forward', more['mix']),
             ('(b) pw_actor_fused + sampling + pw_critic_forward', fused)]
    actor_paths = [('stock ActorNetwork forward', more['actor_stock']), ('FusedActor.logits (pw_actor_fused)', more['actor_fused'])]
    lines = []
    for title, group in (('TD target of a batch', paths), ('the target actor alone, logits [b, N, 5]', actor_paths)):
        for _ in range(20):
            for _, fn in group:
                fn()
        torch.cuda.synchronize()
        t = {name: [] for name, _ in group}
        for _ in range(REPEATS):
            for name, fn in group:
                t[name].append(device_time_us(fn, args.iters))
        lines.append('%s, N = %d, D = %d, b = %d: device-event us per call (%d calls per repeat, %d repeats, paths alternating)' % (
            title, N, D, B, args.iters, REPEATS))
        for name, fn in group:
            v = t[name]
            lines.append('  %-52s mean %8.1f  min %8.1f  max %8.1f  launches %-4s [%s]' % (
                name, sum(v) / len(v), min(v), max(v), launches(fn), ' '.join('%.1f' % x for x in v)))
        if group is paths:
            m, b = t[paths[1][0]], t[paths[2][0]]
            gain, spread = sum(m) / len(m) - sum(b) / len(b), max(m) - min(m)
            ok = gain > spread
            lines.append('  condition: (m) - (b) = %.1f us against the spread of (m)\'s repeats %.1f us: %s' % (
                gain, spread, 'met' if ok else 'NOT met'))
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    return 0 if ok else 1


def bicnet_rows(args):
    """The per-step critic: the TD-target table, then the critic kernel alone beside the attention kernel at N = 48 / 64."""
    from multiagent_rl_amd.critic import BiCNetCritic, CriticNetwork, FusedCritic
    lines = ['BiCNet TD target of a batch (per-agent r, d, y [b, N]), b = %d, D = min(4 + 2 N, 104), A = 5: device-event us per call '
             '(%d calls per repeat, %d repeats, paths alternating)' % (B, args.iters, REPEATS),
             '(a) stock PyTorch-ROCm: target_actor, hard Gumbel one-hot, BiCNetCritic, y;  (b) pw_actor_fused + the same sampling + '
             'pw_critic_forward_steps with the epilogue',
             '%-4s %-5s %-38s %-38s %-8s %-26s %s' % ('N', 'D', '(a) mean [min, max]', '(b) mean [min, max]', 'a / b',
                                                     '(a) - (b) | spread of (a)', 'launches a | b')]
    for N in (3, 6, 12, 24, 48, 64):
        D = min(4 + 2 * N, 104)
        stock, fused, _ = make_paths(N, D, bicnet=True)
        for _ in range(20):
            stock()
            fused()
        torch.cuda.synchronize()
        ta, tb = [], []
        for _ in range(REPEATS):
            ta.append(device_time_us(stock, args.iters))
            tb.append(device_time_us(fused, args.iters))
        ma, mb = sum(ta) / REPEATS, sum(tb) / REPEATS
        lines.append('%-4d %-5d %8.1f [%8.1f, %8.1f] %9s %8.1f [%8.1f, %8.1f] %9s %-8.2f %8.1f | %-15.1f %s | %s' % (
            N, D, ma, min(ta), max(ta), '', mb, min(tb), max(tb), '', ma / mb, ma - mb, max(ta) - min(ta), launches(stock), launches(fused)))
    lines.append('')
    lines.append('FusedCritic.q alone (index actions): the per-step kernel (pw_critic_forward_steps, 16 rows per workgroup for every N) beside the '
                 'attention kernel (pw_critic_forward, 8 rows per workgroup for N > 32): device-event us per call; b = %d is %d / %d workgroups '
                 'on the chip, b = %d fills it' % (B, B // 16, B // 8, 8 * B))
    for b in (B, 8 * B):
        for N in (48, 64):
            D = min(4 + 2 * N, 104)
            torch.manual_seed(N)
            fs, fa = FusedCritic(BiCNetCritic(D + 5, 1).cuda().eval()), FusedCritic(CriticNetwork(D + 5, 1).cuda().eval())
            s1 = torch.randn(b, N, D, device='cuda')
            idx = torch.randint(0, 5, (b, N), device='cuda', dtype=torch.int32)
            group = [('per-step', lambda: fs.q(s1, idx)), ('attention', lambda: fa.q(s1, idx))]
            for _ in range(20):
                for _, fn in group:
                    fn()
            torch.cuda.synchronize()
            t = {name: [] for name, _ in group}
            for _ in range(REPEATS):
                for name, fn in group:
                    t[name].append(device_time_us(fn, args.iters))
            lines.append('  b = %-5d N = %-3d D = %-4d %s' % (b, N, D, '   '.join('%s mean %7.1f [%7.1f, %7.1f]' % (
                name, sum(v) / len(v), min(v), max(v)) for name, v in t.items())))
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    return 0


def make_model_paths(N, D):
    """The no-gradient half of model_ddpg_gumbel_fix.py:150-163."""
    from multiagent_rl_amd.critic import FusedCritic, ModelCriticNetwork
    from multiagent_rl_amd.policy import FusedActor, ModelActorNetwork
    torch.manual_seed(N)
    actor, critic = ModelActorNetwork(D, 5).cuda().eval(), ModelCriticNetwork(D + 5, 1).cuda().eval()
    s1 = torch.randn(B, N, D, device='cuda')
    r, d = torch.randn(B, device='cuda'), (torch.rand(B, device='cuda') < 0.1).float()
    fused_actor, fc = FusedActor(actor), FusedCritic(critic)

    def sample(logits):
        return F.gumbel_softmax(logits.reshape(B * N, -1), hard=True).reshape(B, N, -1)

    @torch.no_grad()
    def stock():
        logits1, _ = actor(s1)
        q_next, _ = critic(s1, sample(logits1))
        return r + GAMMA * torch.squeeze(q_next) * (1. - d)

    @torch.no_grad()
    def fused():
        return fc.td_target(s1, sample(fused_actor.logits(s1)), r, d, GAMMA)
    return stock, fused


def model_rows(args):
    """The model-learning variant: the TD-target table, then ModelTrainer.optimize() unpatched against all four switches at N = 6."""
    import madr_learner
    from multiagent_rl_amd import make_batched_env
    from multiagent_rl_amd.critic import ModelCriticNetwork
    from multiagent_rl_amd.policy import ActorNetwork, FusedActor, ModelActorNetwork, accelerate_trainer
    from multiagent_rl_amd.replay_buffer import ReplayBuffer
    lines = ['Model-learning variant, TD target of a batch, b = %d, D = 4 + 2 N, A = 5: device-event us per call (%d calls per repeat, '
             '%d repeats, paths alternating)' % (B, args.iters, REPEATS),
             '(a) stock PyTorch-ROCm: ModelActorNetwork, hard Gumbel one-hot, ModelCriticNetwork, y;  (b) pw_actor_fused + the same '
             'sampling + pw_critic_forward_model with the epilogue (r_pred = NULL)',
             '%-4s %-5s %-38s %-38s %-8s %-26s %s' % ('N', 'D', '(a) mean [min, max]', '(b) mean [min, max]', 'a / b',
                                                     '(a) - (b) | spread of (a)', 'launches a | b')]
    for N in (3, 6, 12, 24):
        D = 4 + 2 * N
        stock, fused = make_model_paths(N, D)
        for _ in range(20):
            stock()
            fused()
        torch.cuda.synchronize()
        ta, tb = [], []
        for _ in range(REPEATS):
            ta.append(device_time_us(stock, args.iters))
            tb.append(device_time_us(fused, args.iters))
        ma, mb = sum(ta) / REPEATS, sum(tb) / REPEATS
        lines.append('%-4d %-5d %8.1f [%8.1f, %8.1f] %9s %8.1f [%8.1f, %8.1f] %9s %-8.2f %8.1f | %-15.1f %s | %s  %s' % (
            N, D, ma, min(ta), max(ta), '', mb, min(tb), max(tb), '', ma / mb, ma - mb, max(ta) - min(ta), launches(stock), launches(fused),
            'gain beyond the spread' if ma - mb > max(ta) - min(ta) else 'gain NOT beyond the spread'))
    lines.append('')
    lines.append('The critic launch alone (index actions, TD-target epilogue), b = %d: device-event us per call, launch overhead included: the '
                 'attention form (pw_critic_forward) beside the model form without and with the reward head' % B)
    from multiagent_rl_amd.critic import CriticNetwork, FusedCritic
    for N in (3, 6, 12, 24):
        D = 4 + 2 * N
        torch.manual_seed(N)
        fa, fm = FusedCritic(CriticNetwork(D + 5, 1).cuda().eval()), FusedCritic(ModelCriticNetwork(D + 5, 1).cuda().eval())
        s1 = torch.randn(B, N, D, device='cuda')
        idx = torch.randint(0, 5, (B, N), device='cuda', dtype=torch.int32)
        r, d = torch.randn(B, device='cuda'), (torch.rand(B, device='cuda') < 0.1).float()
        group = [('attention', lambda: fa.td_target(s1, idx, r, d, GAMMA)), ('model, q and y', lambda: fm.td_target(s1, idx, r, d, GAMMA)),
                 ('model, q, r_pred and y', lambda: fm._run(s1, idx, r, d, GAMMA, want_reward=True))]
        for _ in range(20):
            for _, fn in group:
                fn()
        torch.cuda.synchronize()
        t = {name: [] for name, _ in group}
        for _ in range(REPEATS):
            for name, fn in group:
                t[name].append(device_time_us(fn, args.iters))
        lines.append('  N = %-3d D = %-4d %s' % (N, D, '   '.join('%s mean %6.1f [%6.1f, %6.1f]' % (
            name, sum(v) / len(v), min(v), max(v)) for name, v in t.items())))
    N = 6
    env = make_batched_env('simple_spread', 1024, auto_reset=True, max_episode_len=25, seed=1, n=N)
    env.reset()
    D = env.obs_dim
    memory = ReplayBuffer(int(1e5), N, D, device_index=True)
    torch.manual_seed(0)
    FusedActor(ActorNetwork(D, 5).cuda().eval(), seed=1).rollout(env, 50, out=False, memory=memory)
    trainers = {}
    for name in ('unpatched', 'all four switches'):
        torch.manual_seed(1)
        on = name != 'unpatched'
        tr = madr_learner.ModelTrainer(ModelActorNetwork(D, 5), ModelCriticNetwork(D + 5, 1), memory, batch_size=B, fused_optimizer=on,
                                       fused_lstm=on, fused_attention=on)
        if on:
            accelerate_trainer(tr, targets=True)
        trainers[name] = tr
    res = {k: [] for k in trainers}
    for tr in trainers.values():
        for _ in range(10):
            tr.optimize()
    iters = 30
    for _ in range(REPEATS):
        for name, tr in trainers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                tr.optimize()
            torch.cuda.synchronize()
            res[name].append((time.perf_counter() - t0) / iters * 1e3)
    lines.append('')
    lines.append('examples/madr_learner.py ModelTrainer, simple_spread N = 6, b = %d: wall ms per optimize() (%d calls per repeat)' % (B, iters))
    for name, v in res.items():
        lines.append('  %-28s mean %.3f  min %.3f  max %.3f   [%s]' % (name, sum(v) / len(v), min(v), max(v), ' '.join('%.3f' % x for x in v)))
    a, b = res['unpatched'], res['all four switches']
    gain, spread = sum(a) / len(a) - sum(b) / len(b), max(a) - min(a)
    lines.append('  unpatched - switched = %.3f ms against the spread of the unpatched repeats %.3f ms: the gain %s' % (
        gain, spread, 'counts' if gain > spread else 'does NOT count'))
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    return 0


def learner_times(lines, iters):
    """Wall time per optimize() of the example learner at N = 6, with / without the fused targets."""
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
    trainers = {}
    for name in ('stock', 'fused'):
        torch.manual_seed(1)
        tr = madr_learner.Trainer(ActorNetwork(D, 5), CriticNetwork(D + 5, 1), memory, batch_size=B)
        if name == 'fused':
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
                 '(%d calls per repeat)' % (B, iters))
    for name in ('stock', 'fused'):
        v = res[name]
        lines.append('  %-28s mean %.3f  min %.3f  max %.3f   [%s]' % (
            'accelerate_trainer(targets=True)' if name == 'fused' else 'unpatched', sum(v) / len(v), min(v), max(v),
            ' '.join('%.3f' % x for x in v)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--out', default=None)
    ap.add_argument('--kernel-only', action='store_true', help='200 fused TD targets at --agents and nothing else (for rocprofv3)')
    ap.add_argument('--agents', type=int, default=6, help='N of --kernel-only')
    ap.add_argument('--wide', action='store_true', help='N = 48 (D = 100) alone: three TD-target paths and the actor alone')
    ap.add_argument('--bicnet', action='store_true', help='the per-step (BiCNet) critic: TD-target table at N = 3 .. 64 and the kernel beside '
                                                          "the attention critic's at N = 48 / 64 (a record, not a gate)")
    ap.add_argument('--model', action='store_true', help='the model-learning variant: TD-target table at N = 3 .. 24 and ModelTrainer.optimize() '
                                                         'unpatched against all four switches (a record, not a gate)')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('critic_bench: needs a GPU (no fallback)')
    if args.model:
        return model_rows(args)
    if args.bicnet:
        return bicnet_rows(args)
    if args.wide:
        return wide_rows(args)
    if args.kernel_only:
        fused = make_paths(args.agents, 4 + 2 * args.agents)[1]
        for _ in range(200):
            fused()
        torch.cuda.synchronize()
        return 0
    lines = ['TD target of a batch, b = %d, D = 4 + 2 N, A = 5: device-event us per call (%d calls per repeat, %d repeats, paths '
             'alternating)' % (B, args.iters, REPEATS),
             '%-4s %-5s %-34s %-34s %-8s %s' % ('N', 'D', '(a) stock PyTorch-ROCm  mean [min, max]', '(b) HIP kernels  mean [min, max]',
                                                'a / b', 'launches a | b')]
    verdict = None
    for N in (3, 6, 12, 24, 48):
        D = 4 + 2 * N
        stock, fused, _ = make_paths(N, D)
        for _ in range(20):
            stock()
            fused()
        torch.cuda.synchronize()
        ta, tb = [], []
        for _ in range(REPEATS):
            ta.append(device_time_us(stock, args.iters))
            tb.append(device_time_us(fused, args.iters))
        ma, mb = sum(ta) / REPEATS, sum(tb) / REPEATS
        lines.append('%-4d %-5d %8.1f [%8.1f, %8.1f] %8s %8.1f [%8.1f, %8.1f] %8s %-8.2f %s | %s%s' % (
            N, D, ma, min(ta), max(ta), '', mb, min(tb), max(tb), '', ma / mb, launches(stock), launches(fused), ''))
        if N == 6:
            verdict = (ma - mb, max(ta) - min(ta))
    ok = verdict[0] > verdict[1]
    lines.append('condition at N = 6: (a) - (b) = %.1f us against the spread of (a)\'s repeats %.1f us: %s' % (
        verdict[0], verdict[1], 'met' if ok else 'NOT met'))
    learner_times(lines, 30)
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
