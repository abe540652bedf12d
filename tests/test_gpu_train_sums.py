"""GPU: the order of the learner's ordered sums (multiagent_rl_amd/csrc/pw_train_sums.hpp), pinned bit for bit.

Reference: tests/train_sums_ref.py, the numpy restatement of the scheme (tiles of 16, a workgroup's tiles in ascending order, a
balanced tree over 128 slots; plain and compensated).  Two bias gradients are column sums and nothing else, one through each variant:
db_gate of the dense front (plain) is the column sum of dG, db of the output layers (compensated) the column sum of each head's dOut.
Rows: 1 (one ragged tile), 16 (exactly one tile: the output layers' direct path), 17 (two workgroups), 2049 (129 tiles: a workgroup
owns two).  The inputs are normal float32 numbers, none zero: a signed zero can only come from the padding, which the restatement
pads the same way.  The weight gradients go through the matrix instruction and are not restated here."""
import functools

import numpy as np
import pytest
import torch

from tests import train_sums_ref

pytestmark = pytest.mark.gpu

ROWS = (1, 16, 17, 2049)


@functools.lru_cache(maxsize=None)
def _normals(seed, *shape):
    """Seeded normal float32 numbers, none zero, subnormal or non-finite; computed once and left unchanged."""
    x = np.random.default_rng(seed).standard_normal(shape).astype(np.float32)
    assert np.isfinite(x).all() and (np.abs(x) >= np.finfo(np.float32).tiny).all()
    x.setflags(write=False)
    return x


def _dev(x):
    return torch.from_numpy(x.copy()).cuda()


def _same_bits(got, want, what):
    got = got.cpu().numpy()
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape, what
    bad = np.flatnonzero(got.view(np.int32) != want.view(np.int32))
    assert bad.size == 0, '%s: %d of %d columns differ, first %d: kernel %r restatement %r' % (
        what, bad.size, got.size, bad[0], got[bad[0]], want[bad[0]])


@pytest.mark.parametrize('dirs', [1, 2])
@pytest.mark.parametrize('rows', ROWS)
def test_front_db_gate_has_the_bits_of_the_plain_restatement(rows, dirs):
    from multiagent_rl_amd import dense
    H, d0, d1 = 64 // dirs, 16, 5
    dG = _normals(rows, rows, 256)
    x0, x1, hid = (_dev(_normals(rows + 1 + i, rows, n)) for i, n in enumerate((d0, d1, 64)))
    w1 = _dev(_normals(5, 64, d0 + d1))
    w_ih = [_dev(_normals(6 + d, 4 * H, 64)) for d in range(dirs)]
    db_gate = dense.launch_backward(_dev(dG), x0, x1, hid, w1, w_ih, False, False)[3]
    assert len(db_gate) == dirs
    _same_bits(torch.cat(db_gate), train_sums_ref.column_sums(dG, False), 'db_gate rows %d dirs %d' % (rows, dirs))


@pytest.mark.parametrize('widths', [(5,), (5, 10, 104)], ids=lambda w: 'x'.join(str(n) for n in w))
@pytest.mark.parametrize('rows', ROWS)
def test_heads_db_has_the_bits_of_the_compensated_restatement(rows, widths):
    from multiagent_rl_amd import heads
    dOuts = [_normals(rows + 10 + k, rows, n) for k, n in enumerate(widths)]
    x = _dev(_normals(rows + 20, rows, 64))
    weights = [_dev(_normals(30 + k, n, 64)) for k, n in enumerate(widths)]
    db = heads.launch_backward([_dev(d) for d in dOuts], x, weights, False, False)[2]
    for k, d in enumerate(dOuts):
        _same_bits(db[k], train_sums_ref.column_sums(d, True), 'db of head %d, rows %d widths %r' % (k, rows, widths))
