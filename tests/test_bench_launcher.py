"""CPU: ``python bench.py --gpus 2 --steps K --warmup W`` from a plain shell starts its own rank processes
(torch.distributed.run children of a parent that never imports torch) and rank 0 prints ONE JSON line -- the
driver's command line, exercised with ``PW_BENCH_STUB=1`` (gloo, a rollout "env" that launches nothing and torch
stand-ins for the HIP launches of the exchanges; the line says ``data: stub``).  What this covers is the launcher,
the rank plumbing, both exchanges' choreography inside bench.py and the shape of the line; the kernels are
covered by the -m gpu tests.  The runs that read the policy-in-the-loop extra or ``multi_gpu`` pass ``--full``: a plain
run measures the headline only."""
import json
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, extra_env=None, timeout=240):
    env = dict(os.environ, PW_BENCH_STUB='1', PYTHONPATH=ROOT)
    env.pop('RANK', None)
    env.pop('WORLD_SIZE', None)
    env.update(extra_env or {})
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')] + args, env=env, cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout, text=True)
    lines = [l for l in p.stdout.splitlines() if l.startswith('{')]
    return p, lines


@pytest.mark.timeout(300)
@pytest.mark.skipif(torch.cuda.device_count() > 0, reason='CPU-container test (stub kernel, gloo)')
def test_bench_gpus2_self_launch_prints_one_line():
    p, lines = _run(['--full', '--gpus', '2', '--steps', '20', '--warmup', '5', '--envs', '8', '--agents', '3', '--chunk', '50',
                     '--batch-size', '8', '--policy-steps', '100', '--policy-chunk', '50'])
    assert p.returncode == 0, p.stderr[-2000:]
    assert len(lines) == 1, p.stdout
    line = json.loads(lines[0])
    assert line['n_gpus'] == 2 and line['steps'] == 20 and line['warmup'] == 5 and line['scaling'] == 'weak'
    assert line['data'].startswith('stub')
    cfg = line['config']
    assert cfg['batched_env_steps_per_launch'] == 50 and cfg['batched_env_steps_timed'] == 1000
    assert cfg['env_steps_per_step'] == 2 * 8 * 50 and cfg['global_batch'] == 16
    assert '50 batched env steps' in cfg['workload'] and '20 launches timed' in cfg['workload']
    ex = cfg['exchange']
    assert ex['error'] is None and ex['exchanges'] == 20 and ex['rows_ingested_root'] == 20 * 8
    assert abs(line['value'] - 2 * 8 * 50 * 20 / cfg['timed_region_s']) < 1e-6 * line['value']
    assert abs(line['ms_per_step'] - cfg['timed_region_s'] * 1e3 / 20) < 1e-9
    g = line['policy_in_loop']['gather']
    assert g['error'] is None and g['transitions_ingested_root'] == g['expected_transitions'] == 2 * 8 * 100
    assert abs(g['bytes_per_env_step'] - g['bytes_per_chunk_per_rank'] / (50 * 8)) < 1e-9
    assert 'cpu_baseline' not in line  # N = 1 only


@pytest.mark.timeout(400)
@pytest.mark.skipif(torch.cuda.device_count() > 0, reason='CPU-container test (stub kernel, gloo)')
def test_bench_gpus8_c4_shape_self_launch():
    """BASELINE configs[3]'s rank count (8 x a small B): the sampled exchange of the headline and the 7-receive full gather
    of the policy extra at the real fan-in, rank-ordered ingest, and the N > 1 line's top-level exchange summary."""
    p, lines = _run(['--full', '--gpus', '8', '--steps', '6', '--warmup', '2', '--envs', '4', '--agents', '3', '--chunk', '50',
                     '--batch-size', '16', '--policy-steps', '100', '--policy-chunk', '50'], timeout=380)
    assert p.returncode == 0, p.stderr[-2000:]
    assert len(lines) == 1, p.stdout
    line = json.loads(lines[0])
    assert line['n_gpus'] == 8 and line['config']['global_batch'] == 32 and line['config']['parallelism'] == 'env-shard x8'
    ex = line['config']['exchange']
    assert ex['error'] is None and ex['exchanges'] == 6 and ex['rows_ingested_root'] == 6 * 16
    g = line['policy_in_loop']['gather']
    assert g['error'] is None and g['transitions_ingested_root'] == g['expected_transitions'] == 8 * 4 * 100
    mg = line['multi_gpu']
    assert mg['full_gather']['transitions_ingested_root'] == mg['full_gather']['expected_transitions'] == 8 * 4 * 100
    assert mg['full_gather']['GBps_per_link'] == g['GBps_per_link'] and mg['full_gather']['peers'] == 7
    assert mg['full_gather']['root_receive_bytes'] == 3 * 7 * g['bytes_per_chunk_per_rank']      # three slots of one block per peer
    assert mg['sampled_exchange']['value_without_exchange'] > 0 and mg['sampled_exchange']['launches_timed'] == 6
    assert abs(mg['sampled_exchange']['value_with_exchange'] - line['value']) < 1e-6 * line['value']


@pytest.mark.timeout(300)
@pytest.mark.skipif(torch.cuda.device_count() > 0, reason='CPU-container test (stub kernel, gloo)')
def test_bench_under_torchrun_env_does_not_relaunch():
    """Started by the driver's own torch.distributed.run (RANK set): no second launcher, one rank = one process."""
    p, lines = _run(['--full', '--gpus', '1', '--steps', '3', '--warmup', '1', '--envs', '4', '--agents', '3', '--chunk', '25',
                     '--policy-steps', '50', '--policy-chunk', '25'],
                    extra_env=dict(RANK='0', LOCAL_RANK='0', WORLD_SIZE='1', PW_BENCH_FORCE_DIST='1',
                                   MASTER_ADDR='127.0.0.1', MASTER_PORT='29577'))
    assert p.returncode == 0, p.stderr[-2000:]
    line = json.loads(lines[0])
    assert line['n_gpus'] == 1 and line['config']['exchange']['exchanges'] == 3
    assert line['policy_in_loop']['gather']['transitions_ingested_root'] == 4 * 50


@pytest.mark.timeout(300)
@pytest.mark.skipif(torch.cuda.device_count() > 0, reason='CPU-container test (stub kernel, gloo)')
def test_a_dying_peer_in_the_policy_extra_does_not_cost_the_line():
    """Rank 1 fails inside the full-gather extra; the root would wait for its block for ever.  The failing rank flags it in
    the process group's store, the root's watchdog prints the (already measured) headline line with that error within a
    second -- not after the policy timeout -- and the run exits NON-ZERO: a run that did not finish is not a success."""
    p, lines = _run(['--full', '--gpus', '2', '--steps', '4', '--warmup', '1', '--envs', '8', '--agents', '3', '--chunk', '50',
                     '--batch-size', '8', '--policy-steps', '400', '--policy-chunk', '50', '--policy-timeout', '60',
                     '--exit-timeout', '4'], extra_env=dict(PW_BENCH_STUB_FAIL_RANK='1'), timeout=200)
    assert p.returncode != 0, 'a run with a dead peer must not report success'
    assert len(lines) == 1, p.stdout
    line = json.loads(lines[0])           # strict JSON: no NaN
    assert line['n_gpus'] == 2 and line['value'] > 0 and line['config']['exchange']['error'] is None
    err = line['policy_in_loop']['error']
    assert 'did not finish' in err and 'rank 1' in err and 'injected failure' in err


@pytest.mark.timeout(300)
@pytest.mark.skipif(torch.cuda.device_count() > 0, reason='CPU-container test (stub kernel, gloo)')
def test_a_hung_policy_extra_times_out_with_the_line_and_a_nonzero_code():
    """The same, but the store flag never arrives (the peer hangs instead of raising): the watchdog's deadline prints the
    line and the exit code is non-zero."""
    p, lines = _run(['--full', '--gpus', '2', '--steps', '4', '--warmup', '1', '--envs', '8', '--agents', '3', '--chunk', '50',
                     '--batch-size', '8', '--policy-steps', '400', '--policy-chunk', '50', '--policy-timeout', '5',
                     '--exit-timeout', '4'], extra_env=dict(PW_BENCH_STUB_HANG_RANK='1'), timeout=200)
    assert p.returncode != 0
    assert len(lines) == 1, p.stdout
    line = json.loads(lines[0])
    assert line['value'] > 0 and 'did not finish within 5 s' in line['policy_in_loop']['error']


def test_profiler_preload_refuses_the_rank_launcher():
    """bench.py --gpus N from a process a profiler has already GPU-initialised must not exec the launcher."""
    p, lines = _run(['--gpus', '2', '--steps', '2'], extra_env=dict(LD_PRELOAD='librocprofiler-sdk-tool.so'))
    assert p.returncode != 0 and not lines
    assert 'profiler preload' in p.stderr and 'PW_BENCH_FORCE_DIST=1' in p.stderr


def test_self_launch_command_line():
    """The child command is torch.distributed.run on 127.0.0.1 with the same arguments; built without torch."""
    sys.path.insert(0, ROOT)
    import bench
    seen = {}
    real = subprocess.call
    try:
        subprocess.call = lambda cmd, env=None: seen.update(cmd=cmd, env=env) or 7
        rc = bench.self_launch(4, ['--gpus', '4', '--steps', '20', '--warmup', '5'])
    finally:
        subprocess.call = real
    cmd = seen['cmd']
    assert rc == 7 and cmd[1:3] == ['-m', 'torch.distributed.run'] and '--nproc-per-node' in cmd
    assert cmd[cmd.index('--nproc-per-node') + 1] == '4' and cmd[cmd.index('--master-addr') + 1] == '127.0.0.1'
    assert cmd[-6:] == ['--gpus', '4', '--steps', '20', '--warmup', '5'] and cmd[-7].endswith('bench.py')
    assert seen['env']['HSA_ENABLE_IPC_MODE_LEGACY'] == '0'


@pytest.mark.timeout(300)
def test_plain_run_is_the_headline_only_and_dumps_the_last_launch(tmp_path):
    """Without --full: the headline's keys, exactly --steps timed launches, none of the extras (CPU baselines, policy in the
    loop, other configurations); --dump-outputs writes the last timed launch's outputs as float .npy files."""
    import numpy as np
    d = tmp_path / 'out'
    p, lines = _run(['--gpus', '1', '--steps', '7', '--warmup', '2', '--envs', '8', '--agents', '3', '--chunk', '50',
                     '--dump-outputs', str(d)])
    assert p.returncode == 0, p.stderr[-2000:]
    assert len(lines) == 1, p.stdout
    line = json.loads(lines[0])
    assert line['steps'] == 7 and line['config']['batched_env_steps_timed'] == 7 * 50
    assert line['unit'] == 'env-steps/s' and line['higher_is_better'] is True and line['dtype'] == 'f32'
    assert abs(line['value'] - 8 * 50 * 7 / line['config']['timed_region_s']) < 1e-6 * line['value']
    assert abs(line['ms_per_step'] - line['config']['timed_region_s'] * 1e3 / 7) < 1e-9
    for extra in ('cpu_baseline', 'policy_in_loop', 'other_configs', 'other_configs_summary', 'multi_gpu'):
        assert extra not in line, extra
    shapes = dict(obs=(400, 3, 10), final_obs=(400, 3, 10), rew=(400, 3), rew_shared=(400,), done=(400, 3), terminal=(400,),
                  step_index=(400,), env_index=(400,))
    assert sorted(os.listdir(str(d))) == sorted(k + '.npy' for k in shapes)
    for k, shape in shapes.items():
        a = np.load(str(d / (k + '.npy')))
        assert a.shape == shape and a.dtype in (np.float32, np.float64), (k, a.shape, a.dtype)
    assert np.array_equal(np.load(str(d / 'step_index.npy')), np.repeat(np.arange(50), 8))
    assert np.load(str(d / 'terminal.npy')).reshape(50, 8)[24::25].all()     # the stub's episode ends


def test_dump_outputs_samples_rows_within_the_budget(tmp_path, monkeypatch):
    """A launch larger than the budget: every env of the last step, a fixed seeded draw of earlier (step, env) rows, the values of
    exactly those rows, final_obs zeroed where no env reset, the same files on every call, and the bound on the bytes written."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    T, B, N, D = 40, 64, 3, 10
    g = torch.Generator().manual_seed(1)
    out = dict(obs=torch.randn(T, B, N, D, generator=g), final_obs=torch.randn(T, B, N, D, generator=g),
               rew=torch.randn(T, B, N, generator=g), rew_shared=torch.randn(T, B, generator=g),
               done=torch.zeros(T, B, N, dtype=torch.bool), terminal=torch.rand(T, B, generator=g) < 0.2)
    monkeypatch.setattr(bench, 'DUMP_BYTES', 100000)
    bench.dump_outputs(str(tmp_path / 'a'), out)
    bench.dump_outputs(str(tmp_path / 'b'), out)
    got = {f[:-4]: np.load(str(tmp_path / 'a' / f)) for f in os.listdir(str(tmp_path / 'a'))}
    for f in os.listdir(str(tmp_path / 'a')):
        assert np.array_equal(got[f[:-4]], np.load(str(tmp_path / 'b' / f)))
    assert sum(os.path.getsize(str(tmp_path / 'a' / f)) for f in os.listdir(str(tmp_path / 'a'))) <= 100000 + 8 * 256
    t, e = got['step_index'].astype(np.int64), got['env_index'].astype(np.int64)
    rows = t * B + e
    assert 2 * B < len(rows) < T * B and np.all(np.diff(rows) > 0)
    assert np.array_equal(rows[-B:], (T - 1) * B + np.arange(B))
    for k in ('obs', 'rew', 'rew_shared', 'terminal'):
        assert np.array_equal(got[k], out[k][t, e].float().numpy()), k
    term = out['terminal'][t, e].numpy()
    assert np.array_equal(got['final_obs'][term], out['final_obs'][t, e].numpy()[term]) and not got['final_obs'][~term].any()


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_dumped_outputs_do_not_depend_on_the_clock_ramp(tmp_path):
    """The real kernel: the last timed launch's outputs are the same whether the untimed clock ramp ran or not (the ramp's own
    episodes advance the episode count every reset draws from, so bench.py must put the state back after it), and final_obs is
    0 wherever no env reset."""
    import numpy as np
    env = dict(os.environ, PYTHONPATH=ROOT)
    env.pop('PW_BENCH_STUB', None)
    dumps = []
    for ramp in ('0', '200'):
        d = str(tmp_path / ('ramp' + ramp))
        p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '2',
                            '--envs', '512', '--chunk', '60', '--ramp-ms', ramp, '--dump-outputs', d], env=env, cwd=ROOT,
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=280, text=True)
        assert p.returncode == 0, p.stderr[-2000:]
        line = json.loads([l for l in p.stdout.splitlines() if l.startswith('{')][0])
        assert line['steps'] == 3 and (line['config']['clock_ramp']['launches'] > 0) == (ramp != '0')
        dumps.append({f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)})
    a, b = dumps
    assert sorted(a) == sorted(b) and a['obs'].shape == (60 * 512, 6, 16)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    term = a['terminal'] != 0
    assert term.any() and np.isfinite(a['obs']).all() and not a['final_obs'][~term].any() and a['final_obs'][term].any()
