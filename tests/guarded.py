"""Device buffers with guard bands, for the tests that hand the library a SUBSET of its optional outputs.

``guarded(shape, dtype)`` is a tensor of ``shape`` that lives inside a larger byte buffer: the view starts on a 256-byte boundary (the
library wants ``obs`` / ``final_obs`` on 16) and at least 256 bytes lie before and after it.  The whole buffer -- the view included --
holds a fixed pattern, a function of the byte's distance from the view's first byte, so two buffers of one shape start out with the
same bytes: what a launch leaves untouched inside the view (``final_obs`` rows of envs that did not reset) compares equal between them.
``assert_guards_intact(view)`` holds the bytes around the view against the pattern and names the first changed one.

A store through a wrong index, or one that survived a missing guard with another output's address, shows here instead of in whatever
the allocator had put next to the tensor.
"""
import numpy as np
import torch

GUARD_BYTES = 256


def _pattern(n, start):
    """Byte i of a buffer whose view starts at byte ``start``: never a run of equal bytes, and none of 0x00 / 0x01 / 0xFF in a row."""
    d = np.arange(n, dtype=np.int64) - start
    return ((d * 197 + 89) & 0xFF).astype(np.uint8)


def guarded(shape, dtype, device='cuda'):
    shape = tuple(int(s) for s in shape)
    nbytes = int(np.prod(shape, dtype=np.int64)) * torch.empty((), dtype=dtype).element_size()
    raw = torch.empty(nbytes + 2 * GUARD_BYTES + 256, dtype=torch.uint8, device=device)
    start = GUARD_BYTES + (-(raw.data_ptr() + GUARD_BYTES)) % 256
    assert (raw.data_ptr() + start) % 256 == 0 and start >= GUARD_BYTES and raw.numel() - (start + nbytes) >= GUARD_BYTES
    raw.copy_(torch.from_numpy(_pattern(raw.numel(), start)))
    view = raw[start:start + nbytes].view(dtype).view(shape)
    assert view.data_ptr() == raw.data_ptr() + start and view.is_contiguous()
    view._guard = (raw, start, nbytes)   # travels with THIS tensor object (not with views or clones of it)
    return view


def assert_guards_intact(view, name='buffer'):
    """Fails naming the first changed guard byte of ``view`` (made by ``guarded``) and its distance from the view."""
    assert hasattr(view, '_guard'), '%s was not made by guarded()' % name
    raw, start, nbytes = view._guard
    got, want = raw.cpu().numpy(), _pattern(raw.numel(), start)
    outside = np.ones(raw.numel(), bool)
    outside[start:start + nbytes] = False
    bad = np.flatnonzero((got != want) & outside)
    if bad.size:
        i = int(bad[0])
        where = '%d bytes before the view' % (start - i) if i < start else '%d bytes past the view\'s last byte' % (i - (start + nbytes) + 1)
        raise AssertionError('%s: %d guard bytes changed; the first is %s (0x%02X, pattern 0x%02X; view of %d bytes)'
                             % (name, bad.size, where, got[i], want[i], nbytes))


def assert_untouched(view, name='buffer'):
    """The view AND its guards still hold the pattern: nothing was written to this buffer at all (a launch that was refused)."""
    assert_guards_intact(view, name)
    raw, start, nbytes = view._guard
    got, want = raw[start:start + nbytes].cpu().numpy(), _pattern(raw.numel(), start)[start:start + nbytes]
    bad = np.flatnonzero(got != want)
    assert not bad.size, '%s: %d of its %d bytes were written; the first at byte %d' % (name, bad.size, nbytes, int(bad[0]))
