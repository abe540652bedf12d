"""CPU: the host side of the per-step (BiCNet) critic and of the per-agent training entry.

(a) tests/bicnet_ref.py (float64 NumPy: the steps of tests/critic_ref.py, then steps @ w2 + b2) reproduces the float64 outputs the
    REFERENCE's BiCNet CriticNetwork gave on the fixture rows (tests/golden/bicnet_critic_forward.npz, made by
    tests/golden/make_bicnet_golden.py) to 1e-12.
(b) ``multiagent_rl_amd.critic.BiCNetCritic`` loads every fixture state_dict with ``strict=True`` and reproduces the reference's float32
    outputs to 2e-6 on the CPU (the bar of tests/test_critic_host.py).
(c) ``pw_critic_forward_steps`` is exported and refuses what ``pw_critic_forward`` refuses, before anything is launched.
(d) ``critic_steps_lds`` (tests/lds_layout_dump_critic_steps.hip, compiled for the host alone): every region aligned, disjoint and inside
    ``bytes`` for N = 1 .. 64, ``bytes`` <= 160 KiB, and the launch sizes of the tested shapes are those of
    tests/golden/lds_bytes_critic_steps.json, worked out by hand from the region list (24 576 + 64 N bytes), never from the function.
(e) ``train_batched(per_agent_transition=True)`` builds a ``per_agent`` ring and refuses ``gather=`` and ``ring='state'``.
"""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import bicnet_ref as br
from tests import critic_ref as cr

torch = pytest.importorskip('torch')

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
G = np.load(os.path.join(HERE, 'golden', 'bicnet_critic_forward.npz'))
CASES = cr.GOLDEN_CASES
IDS = [cr.golden_name(*c) for c in CASES]
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
LDS_MAX = 160 * 1024

needs_hipcc = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which(HIPCC)), reason='hipcc not installed')


def fixture_state_dict(name):
    pre = name + '/sd/'
    return {k[len(pre):]: torch.from_numpy(G[k]) for k in G.files if k.startswith(pre)}


def test_fixture_holds_the_four_cases_and_the_reference_keys():
    for (N, D, heads), name in zip(CASES, IDS):
        assert sorted(fixture_state_dict(name)) == sorted(br.KEYS)
        assert G[name + '/q32'].shape == (cr.GOLDEN_ROWS, N, 1) and G[name + '/q32'].dtype == np.float32
        assert G[name + '/q64'].shape == (cr.GOLDEN_ROWS, N, 1) and G[name + '/q64'].dtype == np.float64
        obs, idx = cr.golden_inputs(N, D, heads)
        want = G[name + '/input_sum']
        assert obs.astype(np.float64).sum() == want[0] and float(idx.sum()) == want[1]
    assert os.path.getsize(os.path.join(HERE, 'golden', 'bicnet_critic_forward.npz')) < (1 << 20)


@pytest.mark.parametrize('N,D,heads', CASES, ids=IDS)
def test_float64_restatement_reproduces_the_reference(N, D, heads):
    name = cr.golden_name(N, D, heads)
    obs, idx = cr.golden_inputs(N, D, heads)
    q = br.forward_f64(fixture_state_dict(name), obs, cr.one_hot(idx, heads))
    assert q.shape == (cr.GOLDEN_ROWS, N)
    err = float(np.abs(q - G[name + '/q64'][:, :, 0]).max())
    print('%s: |q_f64 - reference float64| %.3g' % (name, err))
    assert err <= 1e-12


@pytest.mark.parametrize('N,D,heads', CASES, ids=IDS)
def test_host_module_loads_reference_state_dict_and_reproduces_float32(N, D, heads):
    from multiagent_rl_amd.critic import BiCNetCritic
    name = cr.golden_name(N, D, heads)
    net = BiCNetCritic(D + sum(heads), 1).eval()
    sd = fixture_state_dict(name)
    assert {k: tuple(v.shape) for k, v in net.state_dict().items()} == {k: tuple(v.shape) for k, v in sd.items()}
    net.load_state_dict(sd, strict=True)
    obs, idx = cr.golden_inputs(N, D, heads)
    act = cr.one_hot(idx, heads)
    with torch.no_grad():
        q = net(torch.from_numpy(obs), torch.from_numpy(act)).numpy()
        if len(heads) == 2:   # a list of per-head one-hots is concatenated as the reference does
            parts = [torch.from_numpy(act[..., :heads[0]]), torch.from_numpy(act[..., heads[0]:])]
            assert np.array_equal(net(torch.from_numpy(obs), parts).numpy(), q)
    assert q.shape == (cr.GOLDEN_ROWS, N, 1)
    err = float(np.abs(q - G[name + '/q32']).max())
    print('%s: |q - reference float32| %.3g' % (name, err))
    assert err <= 2e-6


def test_critic_forward_steps_arguments_are_checked_on_the_host():
    """The table of test_critic_forward_arguments_are_checked_on_the_host (tests/test_critic_host.py) on the new entry point: PW_EINVAL
    with a text, nothing launched (no GPU needed; the pointers are fakes)."""
    from multiagent_rl_amd import _lib
    lib = _lib.load()
    assert 'pw_critic_forward_steps' in _lib.SIGNATURES and hasattr(lib, 'pw_critic_forward_steps')
    assert lib.pw_version() >= 111
    p = C.c_void_p(4096)
    w = [p] * 8

    def call(obs=p, idx=p, vec=None, n0=5, n1=0, weights=w, b=64, N=6, D=16, rew=None, done=None, q=p, y=None):
        return lib.pw_critic_forward_steps(obs, idx, vec, n0, n1, *weights, b, N, D, rew, done, 0.95, q, y, None)

    def refused(text, **kw):
        assert call(**kw) == -1, kw
        assert text in lib.pw_last_error(), (kw, lib.pw_last_error())

    refused(b'null', obs=None)
    refused(b'null', q=None)
    for i in range(8):
        refused(b'null', weights=[None if j == i else p for j in range(8)])
    refused(b'exactly one', idx=p, vec=p)
    refused(b'exactly one', idx=None, vec=None)
    refused(b'action widths', n0=0)
    refused(b'action widths', n1=-1)
    refused(b'action widths', n0=9, n1=8)
    refused(b'N must be', N=0)
    refused(b'N must be', N=65)
    refused(b'obs_dim', D=0)
    refused(b'obs_dim', D=105)
    refused(b'b must be', b=0)
    refused(b'b must be', b=1 << 31)
    refused(b'TD target', y=p)
    refused(b'TD target', rew=p, done=p)
    refused(b'TD target', rew=p, y=p)
    refused(b'TD target', done=p, y=p)


@pytest.fixture(scope='module')
def layouts(tmp_path_factory):
    """-> {key: (bytes, [(name, align, alias, offset, size), ...])}"""
    from multiagent_rl_amd import build_native
    src = os.path.join(HERE, 'lds_layout_dump_critic_steps.hip')
    exe = str(tmp_path_factory.mktemp('lds') / 'lds_layout_dump_critic_steps')
    r = subprocess.run([HIPCC, '--offload-host-only', '-std=c++17', '-O1', '-I', os.path.join(build_native.HERE, 'csrc'),
                        '-I', os.path.join(ROOT, 'include'), '-o', exe, src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    res = {}
    for line in out.splitlines():
        key, nbytes, sig, nums = line.split('\t')
        nums = list(map(int, nums.split()))
        regions = [(n, int(a), al == '1', nums[2 * i], nums[2 * i + 1]) for i, (n, a, al) in enumerate(s.split(':') for s in sig.split(','))]
        assert key not in res, key
        res[key] = (int(nbytes), regions)
    return res


@needs_hipcc
def test_steps_layout_is_aligned_disjoint_and_inside_160_kib(layouts):
    assert sorted(layouts) == sorted('critic_steps N=%d R=16' % N for N in range(1, 65))
    for key, (nbytes, regions) in layouts.items():
        assert nbytes <= LDS_MAX, (key, nbytes)
        assert [r[0] for r in regions] == ['out', 'x', 'q'] and not any(r[2] for r in regions)
        for name, align, alias, off, size in regions:
            assert off % align == 0, '%s: region %s is not %d-byte aligned' % (key, name, align)
            assert off + size <= nbytes, '%s: region %s ends past the launch size' % (key, name)
        for i, a in enumerate(regions):
            for b in regions[i + 1:]:
                assert a[3] + a[4] <= b[3] or b[3] + b[4] <= a[3], '%s: regions %s and %s overlap' % (key, a[0], b[0])


@needs_hipcc
def test_steps_launch_sizes_are_the_pinned_ones(layouts):
    with open(os.path.join(HERE, 'golden', 'lds_bytes_critic_steps.json')) as f:
        golden = json.load(f)
    assert len(golden) == 7
    assert {k: layouts[k][0] for k in golden} == golden
    assert golden['critic_steps N=64 R=16'] == 24576 + 64 * 64      # two slots (8 KiB) + four x1 buffers (16 KiB) + [16][N] floats


class _Args(object):
    max_episode_len, num_episodes, is_training = 25, 32, True
    batch_size, warmup_steps, update_rate, save_rate, display = 8, 1024, 100, 32, False


def test_train_batched_builds_a_per_agent_ring_and_refuses_what_is_not_served(tmp_path, monkeypatch):
    """The control flow without a GPU, as tests/test_train_entry.py drives it (stub Trainer, stub rollout through make_rollout=); the
    ring's constructor is recorded instead of run (the real one allocates device memory)."""
    from multiagent_rl_amd import replay_buffer
    from multiagent_rl_amd.train import train_batched
    from tests.test_train_entry import _StubEnv, _StubFused, _StubRollout, _StubTrainer
    built = []

    class _Ring(object):
        def __init__(self, size, num_agents=None, obs_dim=None, **kw):
            built.append(dict(kw, size=size, num_agents=num_agents, obs_dim=obs_dim))
            self.n, self.per_agent = 0, kw.get('per_agent')

        def __len__(self):
            return self.n

    monkeypatch.setattr(replay_buffer, 'ReplayBuffer', _Ring)
    trace = []
    _StubTrainer.trace = trace
    seen = []

    def make_rollout(env, actor, memory, seed):
        seen.append(memory)
        return _StubFused(trace), _StubRollout(env, memory, trace)

    kw = dict(arglist=_Args(), out_dir=str(tmp_path), log=lambda *a: None, chunk=10, make_rollout=make_rollout)
    hist = train_batched(_StubEnv(), 'actor', 'critic', _StubTrainer, 'simple_spread', 'Discrete', per_agent_transition=True, **kw)
    assert hist['stats']['episodes'] == 32
    assert built == [dict(size=int(1e6), num_agents=3, obs_dim=10, device_index=True, per_agent=True)]
    assert isinstance(seen[0], _Ring) and seen[0].per_agent is True
    built.clear()
    train_batched(_StubEnv(), 'actor', 'critic', _StubTrainer, 'simple_spread', 'Discrete', **kw)      # the default is the shared ring
    assert built == [dict(size=int(1e6), num_agents=3, obs_dim=10, device_index=True)]
    built.clear()
    with pytest.raises(ValueError, match='per_agent_transition=True with gather='):
        train_batched(_StubEnv(), 'actor', 'critic', _StubTrainer, 'simple_spread', 'Discrete', per_agent_transition=True,
                      gather=object(), **kw)
    with pytest.raises(ValueError, match="per_agent_transition=True with ring='state'"):
        train_batched(_StubEnv(), 'actor', 'critic', _StubTrainer, 'simple_spread', 'Discrete', per_agent_transition=True,
                      ring='state', **kw)
    assert not built
