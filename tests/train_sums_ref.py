"""The ordered sums of the learner's gradient kernels (multiagent_rl_amd/csrc/pw_train_sums.hpp) restated in numpy: float32,
additions and subtractions only, vectorised over the columns, in the kernels' order -- so a column sum taken here has the kernels' bits.

    rows -> padded with +0.0 to tiles of 16 -> per tile a balanced tree over its 16 rows (rows 2 i and 2 i + 1 first)
         -> a workgroup's tiles added in ascending order into one running sum (its slot)
         -> the slots padded with +0.0 to 128 -> a balanced tree over the slots (slots 2 i and 2 i + 1 first)

The compensated variant carries two-sum pairs (hi, lo) through the same trees, lo starting at 0, and ends in hi + lo; with one
workgroup the result is hi + lo of the running pair and there is no slot tree (the output layers' direct case)."""
import numpy as np

TILE, SLOTS = 16, 128
F32 = np.float32


def split(rows):
    """-> (tiles, tiles per workgroup, workgroups): train_split."""
    tiles = -(-rows // TILE)
    per_group = -(-tiles // SLOTS)
    return tiles, per_group, -(-tiles // per_group)


def two_sum(hi, lo, b_hi, b_lo):
    """(hi, lo) + (b_hi, b_lo): train_two_sum."""
    s = hi + b_hi
    bb = s - hi
    err = (hi - (s - bb)) + (b_hi - bb)
    return s, (lo + b_lo) + err


def _tree(hi, lo):
    """The balanced tree over axis 0 (a power of two long), entries 2 i and 2 i + 1 first; lo None: plain."""
    while hi.shape[0] > 1:
        if lo is None:
            hi = hi[0::2] + hi[1::2]
        else:
            hi, lo = two_sum(hi[0::2], lo[0::2], hi[1::2], lo[1::2])
    return hi[0], None if lo is None else lo[0]


def column_sums(x, compensated):
    """x [rows, cols] float32 -> [cols] float32: every column's sum over the rows, in the kernels' order."""
    assert x.dtype == F32 and x.ndim == 2
    rows, cols = x.shape
    tiles, per_group, groups = split(rows)
    padded = np.zeros((tiles * TILE, cols), F32)
    padded[:rows] = x
    padded = padded.reshape(tiles, TILE, cols)
    slots_hi, slots_lo = np.zeros((SLOTS, cols), F32), np.zeros((SLOTS, cols), F32)
    for g in range(groups):
        hi, lo = np.zeros(cols, F32), np.zeros(cols, F32)
        for t in range(g * per_group, min((g + 1) * per_group, tiles)):
            if compensated:
                hi, lo = two_sum(hi, lo, *_tree(padded[t], np.zeros((TILE, cols), F32)))
            else:
                hi = hi + _tree(padded[t], None)[0]
        slots_hi[g], slots_lo[g] = hi, lo
    if not compensated:
        return _tree(slots_hi, None)[0]
    if groups == 1:
        return slots_hi[0] + slots_lo[0]
    hi, lo = _tree(slots_hi, slots_lo)
    return hi + lo
