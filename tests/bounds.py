"""Guarded device buffers for the tests that hold an entry point to its output bounds (helper module, no tests).

A buffer is one allocation of GUARD + window + GUARD bytes.  The window -- exactly the bytes the entry point may read or write -- starts
`offset` bytes (0..15) behind a 256-byte boundary.  Every byte of the allocation holds one fill value, the window included; an input's
window is then overwritten with its data.  After the call and one synchronise the allocation is copied back and checked ON THE HOST, in
plain numpy (the check_* functions below; tests/test_bounds_helper.py feeds them simulated results):

  guards      every byte outside the window still holds the fill, else BoundsError with the first eight offending offsets, counted from
              the window's first byte (negative: in front of it)
  inputs      the window is byte-identical to what was uploaded, except inside the ranges an in-place entry point is documented to change
  outputs     check_equal against the expected bytes

A case runs once per value of FILLS.  The two fills differ in every byte, so a byte of the window that the kernel never wrote differs from
the expected byte in at least one of the two runs, and a result that depends on a byte outside the input's window changes between them."""
import numpy as np

GUARD = 4096
FILLS = (0xA5, 0x5A)
SLACK = 16                                    # room for the window's offset behind the 256-byte boundary


class BoundsError(AssertionError):
    pass


# ---- host side: plain numpy on host copies ---------------------------------------------------------------------------------------------
def total_bytes(nbytes):
    return GUARD + int(nbytes) + GUARD + SLACK


def window_start(offset):
    assert 0 <= offset < SLACK
    return GUARD + offset


def host_image(nbytes, fill, offset=0, data=None):
    """The allocation as it is uploaded: `fill` everywhere, `data` (nbytes of it) in the window of an input."""
    img = np.full(total_bytes(nbytes), fill, np.uint8)
    if data is not None:
        d = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
        assert len(d) == nbytes, (len(d), nbytes)
        img[window_start(offset): window_start(offset) + nbytes] = d
    return img


def window_of(after, nbytes, offset=0):
    s = window_start(offset)
    return after[s: s + nbytes]


def check_guards(after, nbytes, fill, offset=0, name="buffer"):
    """Every byte outside the window still holds `fill`."""
    s = window_start(offset)
    assert len(after) == total_bytes(nbytes), (name, len(after), nbytes)
    bad = after != fill
    bad[s: s + nbytes] = False
    if bad.any():
        at = np.flatnonzero(bad)
        raise BoundsError("%s: %d byte(s) outside the window of %d bytes were written, first at offsets %s (fill 0x%02X)"
                          % (name, len(at), nbytes, [int(x) - s for x in at[:8]], fill))


def check_input(after, uploaded, fill, offset=0, name="input", may_change=()):
    """Guards intact and the window as uploaded; may_change: (lo, hi) byte ranges of the window an in-place entry point may rewrite."""
    up = np.ascontiguousarray(uploaded).view(np.uint8).reshape(-1)
    check_guards(after, len(up), fill, offset, name)
    diff = window_of(after, len(up), offset) != up
    for lo, hi in may_change:
        diff[lo:hi] = False
    if diff.any():
        at = np.flatnonzero(diff)
        raise BoundsError("%s: %d input byte(s) changed, first at offsets %s" % (name, len(at), [int(x) for x in at[:8]]))


def check_equal(window, want, fill, name="output"):
    """The window against the expected bytes; a differing byte that still holds the fill was never written."""
    want = np.ascontiguousarray(want).view(np.uint8).reshape(-1)
    if len(window) != len(want):
        raise BoundsError("%s: window of %d bytes, %d expected" % (name, len(window), len(want)))
    diff = window != want
    if diff.any():
        at = np.flatnonzero(diff)
        unwritten = int((window[at] == fill).sum())
        raise BoundsError("%s: %d byte(s) differ from the expected ones, first at offsets %s; %d of them still hold the fill 0x%02X (never written)"
                          % (name, len(at), [int(x) for x in at[:8]], unwritten, fill))


def check_untouched(after, fill, name="buffer"):
    """The whole allocation, window included, still holds the fill: nothing was launched on it."""
    bad = after != fill
    if bad.any():
        at = np.flatnonzero(bad)
        raise BoundsError("%s: %d byte(s) were written although the call was refused, first at allocation offsets %s" % (name, len(at), [int(x) for x in at[:8]]))


# ---- device side -------------------------------------------------------------------------------------------------------------------------
class Buf:
    """One guarded allocation on the device.  data: the input's bytes (None: an output of nbytes); ptr: the window's address."""

    def __init__(self, nbytes, fill, offset=0, data=None, name="buffer", may_change=()):
        import torch
        if data is not None:
            data = np.ascontiguousarray(data).view(np.uint8).reshape(-1).copy()
            nbytes = len(data)
        self.nbytes, self.fill, self.offset, self.data, self.name, self.may_change = int(nbytes), fill, offset, data, name, tuple(may_change)
        self.t = torch.from_numpy(host_image(self.nbytes, fill, offset, data)).cuda()
        assert self.t.data_ptr() % 256 == 0, "the allocator's blocks start on 256-byte boundaries"
        self.ptr = self.t.data_ptr() + window_start(offset)

    def after(self):
        return self.t.cpu().numpy()

    def result(self):
        """Host copy of the window, guards (and, for an input, the window) checked.  Call after a synchronise."""
        a = self.after()
        if self.data is not None:
            check_input(a, self.data, self.fill, self.offset, self.name, self.may_change)
        else:
            check_guards(a, self.nbytes, self.fill, self.offset, self.name)
        return window_of(a, self.nbytes, self.offset).copy()

    def expect(self, want):
        check_equal(self.result(), want, self.fill, self.name)

    def untouched(self):
        check_untouched(self.after(), self.fill, self.name) if self.data is None else check_input(self.after(), self.data, self.fill, self.offset, self.name)


def sync():
    """The one synchronise of a case.  A HIP error surfaces here; the session ends with it, so that nothing more is started on a device
    that has faulted."""
    import torch
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        import pytest
        pytest.exit("HIP error at the synchronise, nothing more is run on this device: %s" % e, returncode=3)


def results(*bufs):
    """One synchronise, then every buffer's checked window."""
    sync()
    return [b.result() for b in bufs]
