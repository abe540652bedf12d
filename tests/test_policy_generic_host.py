"""CPU: the host side of the generic one-launch policy rollout (csrc/pw_kernels_policy_generic.hpp, csrc/pworld_policy_generic.hip).

tests/lds_layout_dump_policy_generic.hip, compiled for the host alone, prints policy_generic_lds at every (scenario, observation mode,
N, L, A, E) with rows of at most 64 numbers and E * N <= 96.  Layout: at every shape the host admits, every region starts on the
alignment its widest access needs, regions that are not declared aliases do not overlap, everything ends inside the launch size and
the launch size is at most 160 KB.  Shape search: pw_policy_generic_envs_per_workgroup (host arithmetic, no device) returns the
LARGEST E that fits -- judged from the dumped launch sizes --, admits the families the rollout promises, and returns 0 for rows
longer than 64 numbers."""
import collections
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from multiagent_rl_amd import _lib, build_native

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(build_native.HERE, 'csrc')
INCLUDE = os.path.join(os.path.dirname(build_native.HERE), 'include')
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
LDS_MAX = 160 * 1024
SPREAD, TAG, LOCAL, FULL = 0, 1, 0, 1

pytestmark = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which(HIPCC)), reason='hipcc not installed')


@pytest.fixture(scope='module')
def dump(tmp_path_factory):
    """-> ({(scen, obs, N, L, A): {E: bytes}}, {region signature: (keys, bytes [n], offsets [n, regions], sizes [n, regions])})"""
    src = os.path.join(HERE, 'lds_layout_dump_policy_generic.hip')
    exe = str(tmp_path_factory.mktemp('lds') / 'lds_layout_dump_policy_generic')
    r = subprocess.run([HIPCC, '--offload-host-only', '-std=c++17', '-O1', '-I', CSRC, '-I', INCLUDE, '-o', exe, src],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    sizes, groups = collections.defaultdict(dict), collections.defaultdict(lambda: ([], [], []))
    for line in out.splitlines():
        key, nbytes, sig, nums = line.split('\t')
        scen, obs, N, L, A, E = map(int, re.match(r'policy_generic scen=(\d+) obs=(\d+) N=(\d+) L=(\d+) A=(\d+) E=(\d+)$', key).groups())
        assert E not in sizes[(scen, obs, N, L, A)], key
        sizes[(scen, obs, N, L, A)][E] = int(nbytes)
        g = groups[sig]
        g[0].append(key); g[1].append(nbytes); g[2].append(nums)
    tables = {}
    for sig, (keys, nbytes, nums) in groups.items():
        a = np.array(' '.join(nums).split(), dtype=np.int64).reshape(len(keys), -1, 2)
        tables[sig] = (keys, np.array(nbytes, dtype=np.int64), a[:, :, 0], a[:, :, 1])
    return dict(sizes), tables


def _search(scen, obs, N, L, A):
    return _lib.load().pw_policy_generic_envs_per_workgroup(scen, obs, N, L, A)


def test_layout_is_aligned_disjoint_and_inside_160_kb_at_every_admitted_shape(dump):
    sizes, tables = dump
    admitted = 0
    for sig, (keys, nbytes, off, size) in tables.items():
        regions = [r.split(':') for r in sig.split(',')]
        fits = nbytes <= LDS_MAX          # every shape the search can return (the next test: it returns no other)
        admitted += int(fits.sum())
        keys = np.array(keys)[fits]; nbytes = nbytes[fits]; off = off[fits]; size = size[fits]
        first = lambda bad: keys[int(np.argmax(bad))]  # noqa: E731
        for i, (name, align, alias) in enumerate(regions):
            bad = off[:, i] % int(align) != 0
            assert not bad.any(), '%s: region %s is not %s-byte aligned' % (first(bad), name, align)
            bad = off[:, i] + size[:, i] > nbytes
            assert not bad.any(), '%s: region %s ends past the launch size' % (first(bad), name)
        plain = [i for i, r in enumerate(regions) if r[2] == '0']
        for n, i in enumerate(plain):
            for j in plain[n + 1:]:
                bad = (off[:, i] < off[:, j] + size[:, j]) & (off[:, j] < off[:, i] + size[:, i]) & (size[:, i] > 0) & (size[:, j] > 0)
                assert not bad.any(), '%s: regions %s and %s overlap' % (first(bad), regions[i][0], regions[j][0])
    assert admitted > 10000


def test_shape_search_returns_the_largest_e_that_fits(dump):
    sizes, _ = dump
    assert len(sizes) > 2000
    for (scen, obs, N, L, A), by_e in sizes.items():
        E = _search(scen, obs, N, L, A)
        fitting = [e for e, b in by_e.items() if b <= LDS_MAX]
        assert E == (max(fitting) if fitting else 0), (scen, obs, N, L, A, E, by_e)
        if E:
            assert 1 <= E <= 16 and E * N <= 96
            assert E + 1 == 17 or (E + 1) * N > 96 or by_e[E + 1] > LDS_MAX
            # the launch size grows with E: nothing between 1 and E is skipped
            assert all(by_e[e] <= by_e[e + 1] for e in range(1, max(by_e)))


def test_the_promised_families_are_admitted():
    for N in range(1, 11):                                   # simple_spread, full observation, N = L = 1 .. 10 (D <= 60)
        assert _search(SPREAD, FULL, N, N, 0) >= 1, N
    for N in range(1, 17):                                   # simple_spread, local observation, N <= 16 with L <= N + 2
        for L in range(0, N + 3):
            assert _search(SPREAD, LOCAL, N, L, 0) >= 1, (N, L)
    for N in range(1, 7):                                    # simple_tag, every roster with N <= 6 and L <= 3
        for A in range(0, N + 1):
            for L in range(0, 4):
                assert _search(TAG, LOCAL, N, L, A) >= 1, (N, L, A)
    assert _search(SPREAD, FULL, 3, 3, 0) == 16 and _search(SPREAD, FULL, 10, 10, 0) == 9     # the row cap: E * N <= 96
    assert _search(SPREAD, LOCAL, 12, 12, 0) == 8 and _search(SPREAD, LOCAL, 7, 7, 0) == 13


def test_rows_longer_than_64_numbers_and_bad_shapes_return_0():
    assert _search(SPREAD, FULL, 11, 11, 0) == 0             # D = 4 + 22 + 40 = 66
    assert _search(SPREAD, LOCAL, 31, 31, 0) == 0            # D = 66
    assert _search(SPREAD, LOCAL, 0, 0, 0) == 0 and _search(SPREAD, LOCAL, 65, 3, 0) == 0
    assert _search(2, LOCAL, 2, 3, 0) == 0 and _search(3, LOCAL, 2, 3, 0) == 0      # the communication scenarios
    assert _search(TAG, LOCAL, 4, 2, 5) == 0 and _search(SPREAD, 2, 3, 3, 0) == 0


def test_the_public_header_declares_the_search_and_policy_form_5():
    hdr = open(os.path.join(INCLUDE, 'pworld.h')).read()
    assert re.search(r'int\s+pw_policy_generic_envs_per_workgroup\(int32_t scenario, int32_t obs_mode, int32_t N, int32_t L, int32_t A\);', hdr)
    lib = _lib.load()
    assert lib.pw_version() >= 109
    cfg, h, d = _lib.PwConfig(), C.c_void_p(), _lib.PwDispatch()
    assert lib.pw_config_default(C.byref(cfg), SPREAD, 4, 3, -1, 0) == 0 and lib.pw_create(C.byref(cfg), C.byref(h)) == 0
    lib.pw_get_dispatch(h, C.byref(d))
    d.policy_form = 5
    assert lib.pw_set_dispatch(h, C.byref(d)) == 0
    d.policy_form = 6
    assert lib.pw_set_dispatch(h, C.byref(d)) == -1 and b'out of range' in lib.pw_last_error()
    lib.pw_destroy(h)
    assert os.path.join(CSRC, 'pworld_policy_generic.hip') in build_native.SRCS
    assert not any('policy_generic' in f for fam in build_native.KERNEL_FAMILIES.values() for f in fam)
