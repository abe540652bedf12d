#!/usr/bin/env python3
"""What the episode log costs per chunk against the path it can replace (MI355X; writes profiles/episode_log.txt):

    python tools/episode_log_bench.py                    # per-chunk wall time, launches and synchronisations, kernel time, end to end
    python tools/episode_log_bench.py --skip-e2e         # without the entry-script runs
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/episode_log_bench.py --kernel-only B N   # its own run

Per chunk (T = 100, 25-step episodes with desynchronised clocks, seeded planes), both paths in ONE process, alternating, 5 repeats:
  host    ``ChunkLedger.absorb`` -- what ``train_batched`` runs today: two cumsum, a float64 scatter_add_, nonzero, fancy indexing,
          two host synchronisations;
  device  ``EpisodeLog.absorb`` plus the one read of its length that ``train_batched`` makes.
A call is timed by the host clock around work that ends in a device synchronise.  ``torch.profiler`` counts the device kernels and
the host synchronisations of one chunk of each path: that part of the comparison is a count, not a time.  The kernel time comes from a
``rocprofv3 --kernel-trace --stats`` child run of its own (``--kernel-only``), beside the bytes the launch must move -- T B (4 N + 1)
read, the entries written -- over 8 TB/s.  End to end: ``examples/train_batched.py`` at B = 4096, N = 6 with a fixed episode budget,
``--ledger host`` and ``--ledger device`` alternating in this session.
"""
import argparse
import csv
import glob
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(4096, 6), (8192, 6), (4096, 48)]     # (B, N): simple_spread C2, simple_tag 4 + 2, simple_spread N = 48
T, EPISODE_LEN, HBM_BYTES_PER_S = 100, 25, 8.0e12
KERNELS = ('pw_episode_log_count_kernel', 'pw_episode_log_offsets_kernel', 'pw_episode_log_slots_kernel', 'pw_episode_log_walk_kernel')


def planes(B, N, chunk, device):
    """Chunk number ``chunk`` of a seeded run: rew [T,B,N] float32 in (-1, 0], terminal [T,B] from 25-step clocks that start at e % 25."""
    import torch
    g = torch.Generator().manual_seed(1000 * B + N + chunk)
    rew = -torch.rand(T, B, N, generator=g)
    t = torch.arange(chunk * T, (chunk + 1) * T)
    term = ((t[:, None] + torch.arange(B)[None, :]) % EPISODE_LEN) == EPISODE_LEN - 1
    return rew.to(device).contiguous(), term.to(device).contiguous()


def mean_spread(xs):
    return sum(xs) / len(xs), (max(xs) - min(xs))


def count_chunk(fn, torch):
    """-> (device kernels, host synchronisations) of one call of fn, from torch.profiler's events; (-1, -1) where this torch has no
    profiler to import.  Any error of the profiled call itself is a GPU error and ends the run."""
    try:
        from torch.profiler import ProfilerActivity, profile
    except ImportError:
        return -1, -1
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    kernels = syncs = 0
    for ev in prof.events():
        name = ev.name
        if str(ev.device_type).endswith('CUDA') and 'memcpy' not in name.lower() and 'memset' not in name.lower():
            kernels += 1
        if name in ('hipStreamSynchronize', 'hipDeviceSynchronize', 'hipEventSynchronize', 'cudaStreamSynchronize',
                    'cudaDeviceSynchronize', 'cudaEventSynchronize') or (name.startswith('hipMemcpy') and 'Async' not in name):
            syncs += 1
    return kernels, syncs - 1                    # without the synchronise that ends the window


def per_chunk(B, N, repeats, calls, out):
    import torch
    from multiagent_rl_amd.train import ChunkLedger, EpisodeLog
    dev = torch.device('cuda', 0)
    chunks = [planes(B, N, c, dev) for c in range(4)]
    capacity = (calls + 4) * 5 * B * (repeats + 2)

    def host_call(led, c):
        led.absorb(*chunks[c % 4])
        torch.cuda.synchronize()

    def device_call(log, c):
        log.absorb(*chunks[c % 4])
        n = len(log)                              # the one read train_batched makes
        torch.cuda.synchronize()
        return n

    led, log = ChunkLedger(B, N, dev), EpisodeLog(B, N, capacity, dev)
    for c in range(4):                            # warm-up of both paths, every chunk shape the window uses
        host_call(led, c)
        device_call(log, c)
    host_ms, dev_ms = [], []
    for r in range(repeats):                      # alternating, in one process
        led.totals, led.by_agent = [], [[] for _ in range(N)]          # the lists would otherwise grow through the run
        t0 = time.perf_counter()
        for c in range(calls):
            host_call(led, c)
        host_ms.append((time.perf_counter() - t0) / calls * 1e3)
        t0 = time.perf_counter()
        for c in range(calls):
            device_call(log, c)
        dev_ms.append((time.perf_counter() - t0) / calls * 1e3)
    hk, hs = count_chunk(lambda: led.absorb(*chunks[0]), torch)      # -1: not counted (no torch.profiler), never guessed
    dk, ds = count_chunk(lambda: (log.absorb(*chunks[0]), len(log)), torch)
    hm, hsp = mean_spread(host_ms)
    dm, dsp = mean_spread(dev_ms)
    verdict = 'clears both spreads' if hm - dm > hsp + dsp else 'does not clear the spread'
    out('B=%d N=%d T=%d  per chunk, %d repeats x %d calls:' % (B, N, T, repeats, calls))
    out('  host   ChunkLedger.absorb          %8.3f ms (spread %.3f, runs %s)  %3d device kernels, %d host synchronisations'
        % (hm, hsp, ' '.join('%.3f' % x for x in host_ms), hk, hs))
    out('  device EpisodeLog.absorb + len()   %8.3f ms (spread %.3f, runs %s)  %3d device kernels, %d host synchronisations'
        % (dm, dsp, ' '.join('%.3f' % x for x in dev_ms), dk, ds))
    out('  difference %.3f ms per chunk: %s' % (hm - dm, verdict))


def kernel_only(B, N, calls=20):
    import torch
    from multiagent_rl_amd.train import EpisodeLog
    dev = torch.device('cuda', 0)
    chunks = [planes(B, N, c, dev) for c in range(4)]
    log = EpisodeLog(B, N, (calls + 1) * 5 * B, dev)
    for c in range(calls):
        log.absorb(*chunks[c % 4])
    torch.cuda.synchronize()
    print('episodes', len(log))


def kernel_time(B, N, out):
    """A rocprofv3 child run of its own (the program goes behind ``--``) -> the four kernels' average durations.  A child that fails or
    runs into its time limit ends the whole run: nothing more is started on a GPU that may have faulted."""
    with tempfile.TemporaryDirectory() as d:
        cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', d, '--', sys.executable, os.path.abspath(__file__),
               '--kernel-only', str(B), str(N)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        if r.returncode != 0:
            raise SystemExit('episode_log_bench: the rocprofv3 child at B=%d N=%d failed (exit %d)\n%s' % (B, N, r.returncode, r.stderr[-2000:]))
        rows = {}
        for path in glob.glob(os.path.join(d, '**', '*kernel_stats.csv'), recursive=True):
            for row in csv.DictReader(open(path)):
                for k in KERNELS:
                    if k in row.get('Name', ''):
                        rows[k] = (int(row['Calls']), float(row['AverageNs']) / 1e3, float(row['MinNs']) / 1e3, float(row['MaxNs']) / 1e3)
    if len(rows) != len(KERNELS):
        out('B=%d N=%d  kernel time: not measured (the trace names %s)' % (B, N, sorted(rows)))
        return
    entries = B * T // EPISODE_LEN
    read, written = T * B * (4 * N + 1), entries * (8 * (N + 1) + 8 + 4)
    slot_plane = 2 * 4 * T * B + T * B          # the slot plane written and read once, the flags read twice more by the scan passes
    total_us = sum(v[1] for v in rows.values())
    floor_us = (read + written) / HBM_BYTES_PER_S * 1e6
    out('B=%d N=%d T=%d  kernel time (rocprofv3 --kernel-trace --stats, its own run, %d launches):' % (B, N, T, rows[KERNELS[0]][0]))
    for k in KERNELS:
        out('  %-34s avg %8.2f us  (min %.2f, max %.2f)' % (k, rows[k][1], rows[k][2], rows[k][3]))
    out('  sum of the four                    %8.2f us;  must move %d B read + %d B written = %.2f us at 8 TB/s (+ %d B of slot plane and '
        'flag re-reads, this arrangement\'s own)' % (total_us, read, written, floor_us, slot_plane))
    out('  the launch runs at %.1f%% of the HBM bound: the walk is one dependent chain of T (shares) or T N (totals) float64 additions per '
        'thread with %d threads in flight, so it is bound by that chain\'s latency, not by bandwidth'
        % (100.0 * floor_us / total_us, B * (N + 1)))


def end_to_end(episodes, repeats, out):
    import pickle
    walls, loops = {'host': [], 'device': []}, {'host': [], 'device': []}
    with tempfile.TemporaryDirectory() as d:
        for r in range(repeats):
            for which in ('host', 'device'):
                cmd = [sys.executable, os.path.join(ROOT, 'examples', 'train_batched.py'), '--scenario', 'simple_spread', '--envs', '4096',
                       '--agents', '6', '--episodes', str(episodes), '--ledger', which, '--out-dir', os.path.join(d, 'Models')]
                t0 = time.perf_counter()
                res = subprocess.run(cmd, capture_output=True, text=True, cwd=d, timeout=900)
                wall = time.perf_counter() - t0
                if res.returncode != 0:     # nothing more is started on a GPU that may have faulted
                    raise SystemExit('episode_log_bench: the --ledger %s run failed (exit %d)\n%s' % (which, res.returncode, res.stderr[-2000:]))
                walls[which].append(wall)
                loops[which].append(pickle.load(open(os.path.join(d, 'Models', 'history_simple_spread_0.pkl'), 'rb'))['stats']['wall_s'])
    hm, hsp = mean_spread(walls['host'])
    dm, dsp = mean_spread(walls['device'])
    out('end to end  examples/train_batched.py --envs 4096 --agents 6 --episodes %d (process wall seconds, start-up included), alternating, '
        '%d runs each:' % (episodes, repeats))
    out('  --ledger host    %7.2f s (spread %.2f, runs %s)' % (hm, hsp, ' '.join('%.2f' % x for x in walls['host'])))
    out('  --ledger device  %7.2f s (spread %.2f, runs %s)' % (dm, dsp, ' '.join('%.2f' % x for x in walls['device'])))
    out('  difference %.2f s: %s' % (hm - dm, 'clears the spread of the host runs' if abs(hm - dm) > hsp else 'does not clear the spread'))
    hm, hsp = mean_spread(loops['host'])
    dm, dsp = mean_spread(loops['device'])
    out('  the training loop alone (stats wall_s: rollouts, ledger, updates; no start-up):')
    out('  --ledger host    %7.3f s (spread %.3f, runs %s)' % (hm, hsp, ' '.join('%.3f' % x for x in loops['host'])))
    out('  --ledger device  %7.3f s (spread %.3f, runs %s)' % (dm, dsp, ' '.join('%.3f' % x for x in loops['device'])))
    out('  difference %.3f s: %s' % (hm - dm, 'clears the spread of the host runs' if abs(hm - dm) > hsp else 'does not clear the spread'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--kernel-only', nargs=2, type=int, metavar=('B', 'N'), help='20 absorb launches and nothing else (for rocprofv3)')
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--calls', type=int, default=20, help='chunks per timed window')
    ap.add_argument('--episodes', type=int, default=131072, help='episode budget of the end-to-end runs (eight 100-step chunks)')
    ap.add_argument('--e2e-repeats', type=int, default=3)
    ap.add_argument('--skip-e2e', action='store_true')
    ap.add_argument('--skip-kernel-time', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'episode_log.txt'))
    args = ap.parse_args()
    if args.kernel_only:
        return kernel_only(*args.kernel_only)
    import torch
    if not torch.cuda.is_available():
        sys.exit('episode_log_bench: needs a GPU (a timing taken elsewhere says nothing)')
    if not args.skip_kernel_time and shutil.which('rocprofv3') is None:     # decided before anything is launched
        sys.exit('episode_log_bench: rocprofv3 is not on PATH (--skip-kernel-time runs without the kernel-time part)')
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)

    out('# tools/episode_log_bench.py on %s' % torch.cuda.get_device_name(0))
    for B, N in SHAPES:
        per_chunk(B, N, args.repeats, args.calls, out)
    if not args.skip_kernel_time:
        for B, N in SHAPES:
            kernel_time(B, N, out)
    if not args.skip_e2e:
        end_to_end(args.episodes, args.e2e_repeats, out)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
