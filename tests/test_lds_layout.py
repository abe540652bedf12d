"""CPU: the LDS layout functions beside the kernels (csrc: smem_lds, spread_duo_lds, roll3_lds, ...), which the kernels carve from and
the host dispatchers size their launches with.

tests/lds_layout_dump.hip, compiled for the host alone, prints every layout at every shape its dispatcher admits: N = 1 .. 64, every L
and A the scenario allows, every envs-per-wave, the duo kernels with and without observation blocks (both chunk widths), S1C = 1 .. 13,
E = 1 .. 16, NP in {N, N | 1}, both head forms, the critic's N x R.  Structure: every region starts on the alignment its widest access
needs, regions that are not declared aliases do not overlap, and everything ends inside the launch size.  Sizes: at the shapes the GPU
tests and the benchmark launch, the launch size is the one in tests/golden/lds_bytes.json -- evaluated from the host expressions of the
commit before the layouts became functions, never from the functions under test."""
import collections
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from multiagent_rl_amd import build_native

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(build_native.HERE, 'csrc')
INCLUDE = os.path.join(os.path.dirname(build_native.HERE), 'include')
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')

pytestmark = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which(HIPCC)), reason='hipcc not installed')


@pytest.fixture(scope='module')
def layouts(tmp_path_factory):
    """-> ({key: bytes}, {(layout, region signature): (keys, bytes [n], offsets [n, regions], sizes [n, regions])})"""
    exe = str(tmp_path_factory.mktemp('lds') / 'lds_layout_dump')
    r = subprocess.run([HIPCC, '--offload-host-only', '-std=c++17', '-O1', '-I', CSRC, '-I', INCLUDE, '-o', exe,
                        os.path.join(HERE, 'lds_layout_dump.hip')], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    total, groups = {}, collections.defaultdict(lambda: ([], [], []))
    for line in out.splitlines():
        key, nbytes, sig, nums = line.split('\t')
        assert key not in total, key
        total[key] = int(nbytes)
        g = groups[(key.split(' ')[0], sig)]
        g[0].append(key); g[1].append(nbytes); g[2].append(nums)
    tables = {}
    for k, (keys, nbytes, nums) in groups.items():
        a = np.array(' '.join(nums).split(), dtype=np.int64).reshape(len(keys), -1, 2)
        tables[k] = (keys, np.array(nbytes, dtype=np.int64), a[:, :, 0], a[:, :, 1])
    return total, tables


LAYOUTS = ['env_generic', 'spread_stream', 'spread_duo', 'spread_quad', 'tag_stream', 'tag_duo', 'actor_front', 'actor_fused', 'actor16',
           'roll3', 'roll3j', 'policy_tag', 'policy_ref', 'critic']


def test_every_layout_is_aligned_disjoint_and_inside_its_launch_size(layouts):
    _, tables = layouts
    assert sorted({k[0] for k in tables}) == sorted(LAYOUTS)
    for (layout, sig), (keys, nbytes, off, size) in tables.items():
        regions = [r.split(':') for r in sig.split(',')]
        first = lambda bad: keys[int(np.argmax(bad))]  # noqa: E731
        assert (nbytes <= 160 * 1024).all(), first(nbytes > 160 * 1024)
        for i, (name, align, alias) in enumerate(regions):
            bad = off[:, i] % int(align) != 0
            assert not bad.any(), '%s: region %s is not %s-byte aligned' % (first(bad), name, align)
            bad = off[:, i] + size[:, i] > nbytes
            assert not bad.any(), '%s: region %s ends past the launch size' % (first(bad), name)
        plain = [i for i, r in enumerate(regions) if r[2] == '0']
        for n, i in enumerate(plain):
            for j in plain[n + 1:]:
                bad = (off[:, i] < off[:, j] + size[:, j]) & (off[:, j] < off[:, i] + size[:, i])
                assert not bad.any(), '%s: regions %s and %s overlap' % (first(bad), regions[i][0], regions[j][0])


def test_launch_sizes_are_those_of_the_commit_before_the_layout_functions(layouts):
    total, _ = layouts
    with open(os.path.join(HERE, 'golden', 'lds_bytes.json')) as f:
        golden = json.load(f)
    assert len(golden) > 500
    missing = [k for k in golden if k not in total]
    assert not missing, missing[:10]
    wrong = {k: (total[k], v) for k, v in golden.items() if total[k] != v}
    assert not wrong, sorted(wrong.items())[:10]
