"""tests/guarded.py on the CPU: the guard bands notice a byte written before or after the view, and nothing written inside it."""
import pytest

torch = pytest.importorskip('torch')

from tests.guarded import GUARD_BYTES, assert_guards_intact, guarded  # noqa: E402


@pytest.mark.parametrize('shape, dtype', [((7, 13, 6, 16), torch.float32), ((7, 13), torch.bool), ((3, 5), torch.int64), ((1,), torch.uint8)])
def test_view_is_aligned_padded_and_patterned_alike(shape, dtype):
    a, b = guarded(shape, dtype, 'cpu'), guarded(shape, dtype, 'cpu')
    for v in (a, b):
        raw, start, nbytes = v._guard
        assert tuple(v.shape) == shape and v.dtype == dtype and v.is_contiguous() and v.data_ptr() % 256 == 0
        assert start >= GUARD_BYTES and raw.numel() - start - nbytes >= GUARD_BYTES
        assert_guards_intact(v)
    assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))      # the same bytes in every buffer of one shape
    a.view(torch.uint8).fill_(0)                                      # the view is the caller's
    assert_guards_intact(a)


@pytest.mark.parametrize('offset, words', [(-1, '1 bytes before the view'), (-GUARD_BYTES, '%d bytes before' % GUARD_BYTES),
                                           (0, "1 bytes past the view's last byte"), (GUARD_BYTES - 1, '%d bytes past' % GUARD_BYTES)])
def test_a_changed_guard_byte_is_named(offset, words):
    v = guarded((5, 3), torch.float32, 'cpu')
    raw, start, nbytes = v._guard
    i = start + offset if offset < 0 else start + nbytes + offset
    raw[i] ^= 0x40
    with pytest.raises(AssertionError, match=words):
        assert_guards_intact(v, 'probe')
    raw[i] ^= 0x40
    assert_guards_intact(v, 'probe')


def test_a_plain_tensor_is_refused():
    with pytest.raises(AssertionError, match='not made by guarded'):
        assert_guards_intact(torch.zeros(3))


def test_untouched_means_the_view_too():
    from tests.guarded import assert_untouched
    v = guarded((4, 3), torch.float32, 'cpu')
    assert_untouched(v)
    v[1, 1] = 0
    with pytest.raises(AssertionError, match='4 of its 48 bytes were written; the first at byte 16'):
        assert_untouched(v, 'probe')
    assert_guards_intact(v, 'probe')
