"""The checker of tests/bounds.py on simulated results, without a GPU: every mistake tests/test_gpu_bounds.py exists for is reported, a
correct result passes."""
import numpy as np
import pytest

import bounds


def simulate(nbytes, fill, offset, want, spoil=None):
    """The output allocation after a kernel that wrote `want` into the window; spoil(after, window start) then applies a mistake."""
    after = bounds.host_image(nbytes, fill, offset)
    s = bounds.window_start(offset)
    after[s: s + nbytes] = want
    if spoil:
        spoil(after, s)
    return after


def verdict(nbytes, offset, want, spoil=None):
    """-> messages of the BoundsErrors over the two fills (empty: both passes are clean)."""
    out = []
    for fill in bounds.FILLS:
        after = simulate(nbytes, fill, offset, want, (lambda a, s: spoil(a, s, fill)) if spoil else None)
        try:
            bounds.check_guards(after, nbytes, fill, offset, "out")
            bounds.check_equal(bounds.window_of(after, nbytes, offset), want, fill, "out")
        except bounds.BoundsError as e:
            out.append(str(e))
    return out


@pytest.mark.parametrize("offset", [0, 2, 6, 8, 15])
@pytest.mark.parametrize("nbytes", [1, 9, 54, 4097])
def test_checker_reports_each_mistake(nbytes, offset):
    rng = np.random.default_rng(nbytes * 16 + offset)
    want = rng.integers(0, 256, nbytes, dtype=np.uint8)
    want[0], want[-1] = bounds.FILLS[0], bounds.FILLS[1]                # expected bytes that equal one of the fills
    assert verdict(nbytes, offset, want) == []                          # a correct result passes, with both fills

    def before(a, s, fill): a[s - 1] = fill ^ 0xFF
    def behind(a, s, fill): a[s + nbytes] = fill ^ 0xFF
    def far_behind(a, s, fill): a[-1] = 0
    def far_before(a, s, fill): a[0] = 0
    for spoil, off in ((before, -1), (behind, nbytes), (far_behind, bounds.total_bytes(nbytes) - 1 - bounds.window_start(offset)), (far_before, -bounds.window_start(offset))):
        msgs = verdict(nbytes, offset, want, spoil)
        assert len(msgs) == 2 and all("outside the window" in m and "[%d]" % off in m for m in msgs), (spoil.__name__, msgs)

    # one byte of the window never written: it keeps the fill, and at least one of the two fills differs from the expected byte --
    # also where the expected byte IS one of the fills (first and last byte here)
    for at in sorted({0, nbytes // 2, nbytes - 1}):
        def unwritten(a, s, fill, at=at): a[s + at] = fill
        msgs = verdict(nbytes, offset, want, unwritten)
        assert 1 <= len(msgs) <= 2 and all("[%d]" % at in m and "1 of them still hold the fill" in m for m in msgs), (at, msgs)

    # a wrong byte (written, but not the expected value) is reported by the same comparison
    def wrong(a, s, fill): a[s + nbytes // 2] = want[nbytes // 2] ^ 0x10
    assert len(verdict(nbytes, offset, want, wrong)) >= 1


def test_checker_reports_eight_offsets_at_most_and_in_order():
    nbytes, offset, fill = 100, 6, bounds.FILLS[0]
    after = bounds.host_image(nbytes, fill, offset)
    s = bounds.window_start(offset)
    after[s - 20: s - 2] = 0
    after[s + nbytes + 3] = 0
    with pytest.raises(bounds.BoundsError) as e:
        bounds.check_guards(after, nbytes, fill, offset, "out")
    assert "19 byte(s)" in str(e.value) and str(list(range(-20, -12))) in str(e.value)


@pytest.mark.parametrize("offset", [0, 2, 8])
def test_checker_reports_changed_input(offset):
    rng = np.random.default_rng(offset)
    data = rng.integers(0, 27, 9 * 50, dtype=np.uint8)
    for fill in bounds.FILLS:
        img = bounds.host_image(len(data), fill, offset, data)
        bounds.check_input(img, data, fill, offset, "in")                               # as uploaded: passes
        s = bounds.window_start(offset)
        bad = img.copy(); bad[s + 17] ^= 1
        with pytest.raises(bounds.BoundsError, match=r"1 input byte\(s\) changed, first at offsets \[17\]"):
            bounds.check_input(bad, data, fill, offset, "in")
        bounds.check_input(bad, data, fill, offset, "in", may_change=[(10, 18)])        # inside the documented range: allowed
        with pytest.raises(bounds.BoundsError, match="input byte"):
            bounds.check_input(bad, data, fill, offset, "in", may_change=[(18, 30)])    # outside it: reported
        bad = img.copy(); bad[s - 1] ^= 1                                               # an "input" written in front of its window
        with pytest.raises(bounds.BoundsError, match="outside the window"):
            bounds.check_input(bad, data, fill, offset, "in")


def test_checker_untouched_and_sizes():
    for fill in bounds.FILLS:
        img = bounds.host_image(64, fill, 0)
        bounds.check_untouched(img, fill, "out")
        img[bounds.window_start(0) + 5] = fill ^ 1                                      # inside the window counts: nothing may be launched
        with pytest.raises(bounds.BoundsError, match="refused"):
            bounds.check_untouched(img, fill, "out")
    with pytest.raises(bounds.BoundsError, match="expected"):
        bounds.check_equal(np.zeros(5, np.uint8), np.zeros(6, np.uint8), 0xA5)
    assert all((a ^ b) == 0xFF for a, b in [bounds.FILLS])                               # the fills differ in every bit
    assert bounds.window_start(6) % 16 == 6 and bounds.GUARD % 256 == 0
