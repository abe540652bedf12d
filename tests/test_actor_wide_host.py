"""CPU: the host side of the actor kernels at observation rows of 65 .. 104 numbers (S1C = ceil(D / 8) = 9 .. 13).

tests/lds_layout_dump_actor_wide.hip, compiled for the host alone, prints actor_lds and actor_front_lds (csrc/pw_kernels_policy.hpp) at
S1 = 4 S1C = 36 .. 52.  Layout: every region starts on the alignment its widest access needs, regions that are not the declared alias
(s_lg = s_g) do not overlap, everything ends inside the launch size and the launch size is at most 160 KiB.  Sizes: the ten launch
sizes are those of tests/golden/lds_bytes_actor_wide.json, worked out by hand from the region list (fused: 132 288 + 512 S1 bytes,
front: 83 712 + 512 S1), never from the functions under test.
Code objects (tools/code_object.py, as tests/test_code_object.py): pw_actor_fused_kernel<9 .. 13> and pw_actor_front_kernel<9 .. 13>
exist, and the fused ones -- 512 threads, two waves per SIMD -- use at most 256 registers per lane.
"""
import json
import os
import re
import shutil
import subprocess
import sys

import pytest

from multiagent_rl_amd import build_native

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(build_native.HERE, 'csrc')
INCLUDE = os.path.join(ROOT, 'include')
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
LDS_MAX = 160 * 1024
WIDE_S1C = (9, 10, 11, 12, 13)

sys.path.insert(0, os.path.join(ROOT, 'tools'))
import code_object  # noqa: E402

needs_hipcc = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which(HIPCC)), reason='hipcc not installed')
needs_llvm = pytest.mark.skipif(not code_object.tools_present(), reason='ROCm LLVM binary tools not installed')


@pytest.fixture(scope='module')
def layouts(tmp_path_factory):
    """-> {key: (bytes, [(name, align, alias, offset, size), ...])}"""
    src = os.path.join(HERE, 'lds_layout_dump_actor_wide.hip')
    exe = str(tmp_path_factory.mktemp('lds') / 'lds_layout_dump_actor_wide')
    r = subprocess.run([HIPCC, '--offload-host-only', '-std=c++17', '-O1', '-I', CSRC, '-I', INCLUDE, '-o', exe, src],
                       capture_output=True, text=True)
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
def test_wide_layouts_are_aligned_disjoint_and_inside_160_kib(layouts):
    assert sorted(layouts) == sorted('%s S1=%d' % (k, 4 * c) for k in ('actor_front', 'actor_fused') for c in WIDE_S1C)
    for key, (nbytes, regions) in layouts.items():
        assert nbytes <= LDS_MAX, (key, nbytes)
        for name, align, alias, off, size in regions:
            assert off % align == 0, '%s: region %s is not %d-byte aligned' % (key, name, align)
            assert off + size <= nbytes, '%s: region %s ends past the launch size' % (key, name)
        plain = [r for r in regions if not r[2]]
        for i, a in enumerate(plain):
            for b in plain[i + 1:]:
                assert a[3] + a[4] <= b[3] or b[3] + b[4] <= a[3], '%s: regions %s and %s overlap' % (key, a[0], b[0])
        by = {r[0]: r for r in regions}
        if key.startswith('actor_fused'):
            assert [r[0] for r in regions if r[2]] == ['lg'] and by['lg'][3] == by['g'][3] and by['lg'][4] <= by['g'][4]   # s_lg = s_g
        else:
            assert not any(r[2] for r in regions)
            assert by['f_w1'][3] == by['f_wih'][3] + by['f_wih'][4]    # one float4 copy loop fills both


@needs_hipcc
def test_wide_launch_sizes_are_the_pinned_ones(layouts):
    with open(os.path.join(HERE, 'golden', 'lds_bytes_actor_wide.json')) as f:
        golden = json.load(f)
    assert len(golden) == 10
    assert {k: v[0] for k, v in layouts.items()} == golden
    assert golden['actor_fused S1=52'] == 158912 and golden['actor_front S1=52'] == 110336


@pytest.fixture(scope='module')
def kernels():
    if not all(os.path.exists(o) for o in build_native.objects()):
        build_native.build(force=True)          # a tree that carries only the .so: the objects are rebuilt
    return code_object.all_kernels()


def _instances(kernels, family):
    out = {}
    for name, d in kernels.items():
        m = re.match(r'(?:void )?%s<(\d+)>\(' % family, name)
        if m:
            out[int(m.group(1))] = d
    return out


@needs_llvm
def test_wide_instantiations_exist_and_the_fused_ones_fit_two_waves_per_simd(kernels):
    fused, front = _instances(kernels, 'pw_actor_fused_kernel'), _instances(kernels, 'pw_actor_front_kernel')
    assert sorted(fused) == list(range(1, 14)), sorted(fused)
    assert sorted(front) == list(range(1, 14)), sorted(front)
    for c in WIDE_S1C:
        # 512 threads = two waves per SIMD: 512 registers per SIMD lane shared by two waves (arch + accumulation)
        assert fused[c]['.vgpr_count'] <= 256, (c, fused[c]['.vgpr_count'])
        for d in (fused[c], front[c]):
            assert d['.vgpr_spill_count'] == 0 and d['scratch_insts'] == 0 and d['.private_segment_fixed_size'] <= 64, (c, d['.vgpr_count'])
