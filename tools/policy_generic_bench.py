#!/usr/bin/env python3
"""The generic one-launch policy rollout (pw_policy_rollout_generic_kernel) against what the library offered for the same envs before
it, on the GPU (there is no fallback: without one this fails).

    python tools/policy_generic_bench.py [--out profiles/policy_generic.txt]
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/policy_generic_bench.py --kernel-only   # its own run

Configurations, B = 4096, max_episode_len = 25, auto-reset: simple_spread with the full observation at N = 3 and N = 6, and
simple_spread N = 5 with per-agent sizes / accelerations / speed clamps (the `mixed` set of tests/world_constants.py; policy_form 5).
Paths:
(a) one launch: BatchedRollout.collect_one_launch, 100-step chunks, ring sink + episode statistics in the same kernel;
(b) per step:   BatchedRollout.collect -- FusedActor() + env.step() + the ring append, three launches per step;
(c) captured:   the same steps captured in a hipGraph (BatchedRollout.capture()), one host call per two steps.
Device events around STEPS batched steps after a 60 ms clock ramp, five repeats per path, the paths alternating.
Sanity anchor: simple_spread N = 6 with the local observation (a fast-path shape), path (a) under policy_form 5 against form 3: what
the generic step costs beside the specialised one.
Exit status 1 if in some configuration (a) is not faster than (b) and (c) by more than the spread (max - min) of that path's repeats.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

B, T, REPEATS, STEPS = 4096, 100, 5, 200
MIXED = dict(size=[0.15, 0.1, 0.2, 0.12, 0.07], accel=[-1.0, 2.5, -1.0, 6.0, 3.0], max_speed=[-1.0, 0.8, -1.0, 1.1, 0.5])


def make_env(name, form=0):
    from multiagent_rl_amd import make_batched_env
    from multiagent_rl_amd.env import BatchedParticleEnv, make_config
    run = dict(auto_reset=True, max_episode_len=25, seed=12345678)
    if name == 'mixed N=5':
        cfg = make_config('simple_spread', B, num_agents=5, action_force_uses_accel=True, **run)
        for i in range(5):
            cfg.agent_size[i], cfg.agent_accel[i], cfg.agent_max_speed[i] = MIXED['size'][i], MIXED['accel'][i], MIXED['max_speed'][i]
        env = BatchedParticleEnv('simple_spread', config=cfg)
    else:
        kind, n = name.split(' N=')
        env = make_batched_env('simple_spread', B, n=int(n), local_observation=kind != 'full', **run)
    if form:
        env.set_dispatch(policy_form=form)
    return env


def make_rollout(name, form=0, capture=False):
    from multiagent_rl_amd.policy import ActorNetwork, FusedActor
    from multiagent_rl_amd.replay_buffer import ReplayBuffer
    from multiagent_rl_amd.rollout import BatchedRollout
    torch.manual_seed(1)
    env = make_env(name, form)
    actor = FusedActor(ActorNetwork(env.obs_dim, 5).cuda().eval(), seed=12345678)
    ro = BatchedRollout(env, actor, ReplayBuffer(int(1e6), env.n, env.obs_dim))
    return ro.capture(2) if capture else ro


def device_time_us_per_step(fn, steps):
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.06:   # clock ramp
        fn(2)
        torch.cuda.synchronize()
    beg, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    beg.record()
    fn(steps)
    end.record()
    end.synchronize()
    return beg.elapsed_time(end) * 1e3 / steps


def fmt(v):
    return '%8.2f [%8.2f, %8.2f] %10.3g' % (sum(v) / len(v), min(v), max(v), B / (sum(v) / len(v)) * 1e6)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--kernel-only', action='store_true', help='ten 100-step launches at full N=3 and nothing else (for rocprofv3)')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('policy_generic_bench: needs a GPU (no fallback)')
    if args.kernel_only:
        ro = make_rollout('full N=3')
        ro.collect_one_launch(10 * T, chunk=T)
        torch.cuda.synchronize()
        return 0
    lines = ['simple_spread, B = %d, device-event us per batched step (%d steps per repeat, %d repeats, paths alternating): mean [min, max] '
             'env-steps/s' % (B, STEPS, REPEATS)]
    ok = True
    for name, form in (('full N=3', 0), ('full N=6', 0), ('mixed N=5', 5)):
        one, loop, graph = make_rollout(name, form), make_rollout(name), make_rollout(name, capture=True)
        paths = (('(a) one launch, T = %d' % T, lambda s: one.collect_one_launch(s, chunk=T)),
                 ('(b) collect, per step', loop.collect), ('(c) collect, hipGraph', graph.collect))
        res = {k: [] for k, _ in paths}
        for _ in range(REPEATS):
            for k, fn in paths:
                res[k].append(device_time_us_per_step(fn, STEPS))
        lines.append('%s (D = %d, %s)' % (name, one.env.obs_dim, one.env.last_kernel()))
        for k, _ in paths:
            lines.append('  %-26s %s' % (k, fmt(res[k])))
        a = res[paths[0][0]]
        for k in (paths[1][0], paths[2][0]):
            v = res[k]
            gain, spread = sum(v) / len(v) - sum(a) / len(a), max(v) - min(v)
            met = gain > spread
            ok = ok and met
            lines.append('  condition against %s: gain %.2f us, spread of its repeats %.2f us: %s' % (k[:3], gain, spread, 'met' if met else 'NOT met'))
    g5, s3 = make_rollout('local N=6', 5), make_rollout('local N=6', 3)
    res = {5: [], 3: []}
    for _ in range(REPEATS):
        res[5].append(device_time_us_per_step(lambda s: g5.collect_one_launch(s, chunk=T), STEPS))
        res[3].append(device_time_us_per_step(lambda s: s3.collect_one_launch(s, chunk=T), STEPS))
    lines.append('sanity anchor, local N=6 (D = 16), one launch, T = %d' % T)
    lines.append('  %-26s %s   (%s)' % ('policy_form 5', fmt(res[5]), g5.env.last_kernel()))
    lines.append('  %-26s %s   (%s)' % ('policy_form 3', fmt(res[3]), s3.env.last_kernel()))
    lines.append('  generic / specialised = %.2f' % (sum(res[5]) / sum(res[3])))
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
