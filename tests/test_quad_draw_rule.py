"""CPU: the quad kernel's reset draws ahead (csrc/pw_kernels_spread_quad.hpp, "Reset draws ahead").

tests/quad_draw_rule_dump.hip, compiled for the host alone, tabulates the one rule by which the kernel's three kinds of waves decide that
a reset step takes its positions from the draws wave OB made ahead -- over the episode length, the steps since the pipeline's start, clocks
equal or apart, and auto_reset -- and this file holds the table against the rule restated here.  The same program runs the draw in the
slices the kernel runs it in and compares every bit with pw_reset_xy, and prints where the entries lie in LDS: in the 16 entries behind the
48 states of a ring slot, each at a place of its own."""
import os
import shutil
import subprocess

import pytest

from multiagent_rl_amd import build_native
from multiagent_rl_amd.env import QUAD_DRAW_DEPTH

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(build_native.HERE, 'csrc')
INCLUDE = os.path.join(os.path.dirname(build_native.HERE), 'include')
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')

pytestmark = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which(HIPCC)), reason='hipcc not installed')


@pytest.fixture(scope='module')
def dump(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('rule') / 'quad_draw_rule_dump')
    r = subprocess.run([HIPCC, '--offload-host-only', '-std=c++17', '-O1', '-ffp-contract=off', '-I', CSRC, '-I', INCLUDE, '-o', exe,
                        os.path.join(HERE, 'quad_draw_rule_dump.hip')], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [ln.split() for ln in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines()]
    return {k: [ln[1:] for ln in lines if ln[0] == k] for k in ('depth', 'rule', 'at', 'draws')}


def test_the_depth_is_the_exported_one(dump):
    (depth, _, slices, _, rounds, _, delay), = dump['depth']
    assert int(depth) == QUAD_DRAW_DEPTH
    assert int(delay) == 1                          # the first slice runs one iteration behind a reset step (the GPU tests' cases assume it)
    assert int(slices) * int(rounds) == 10          # Philox4x32-10, whole rounds per slice
    assert int(depth) == int(slices) + 1            # the entries are written one barrier before the first step that may read them


def test_the_engage_rule_is_the_one_restated_here(dump):
    rows = [tuple(map(int, r)) for r in dump['rule']]
    assert len(rows) == 2 * 31 * 2 * 33
    seen = set()
    for auto_reset, ep_len, equal, since, got in rows:
        want = bool(auto_reset) and ep_len > 0 and bool(equal) and since >= QUAD_DRAW_DEPTH
        assert bool(got) == want, (auto_reset, ep_len, equal, since, got)
        seen.add(want)
    assert seen == {False, True}
    # what follows from it at an episode's start (the pipeline's first slice runs one step behind the reset step, the next reset
    # comes ep_len - 1 steps later): episodes of up to QUAD_DRAW_DEPTH steps never engage, longer ones always
    table = {r[:4]: r[4] for r in rows}
    for ep_len in range(1, 31):
        assert bool(table[(1, ep_len, 1, ep_len - 1)]) == (ep_len > QUAD_DRAW_DEPTH)


def test_the_entries_lie_in_the_ring_slots_unused_tails(dump):
    at = {int(i): int(j) for i, j in dump['at']}
    assert sorted(at) == list(range(48))
    assert len(set(at.values())) == 48
    for j in at.values():   # float2 units from entry 48 of a slot (float2 96 of its 128); a region spans two slots
        k = j + 96
        assert 96 <= k % 128 < 128 and k < 256, j


def test_the_sliced_draw_is_pw_reset_xy_bit_for_bit(dump):
    (n, bad), = dump['draws']
    assert int(n) > 5000 and int(bad) == 0
