"""CPU-side checks of the batched window / image entries (the same window out of N equal frames in one call, N images through the image
front end in one call; include/t3hip.h; no GPU): the plan -- one frame's window plan, which batches run as one decoder launch and one
crop launch, bytes, stride minima and scratch -- the argument limits, that the device entries refuse what is wrong with their arguments
before they ask for a device, and the register budget of the new kernels read from the built objects."""
import os
import sys

import pytest

from test_window_plan import STD_RES, centered_window, units_tile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SINGLE_K = {0: 24, 1: 22, 2: 20, 3: 18}            # profile -> k with uep_uniform(profile)
SLACK = 256                                        # t3hip.h: the single-frame entry's slack behind the run, once per call


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    return ge.load_package()


def r16(x):
    return (x + 15) & ~15


def win_tuple(p):
    return (p.n_tiles, p.tile_lo, p.tile_hi, p.first_px, p.n_px, p.tile_range)


# (fw, fh, x0, y0, w, h) on a stream of 100 x 70 pixels
WINDOWS = [(100, 70, 0, 0, 100, 70), (100, 70, 10, 22, 50, 20), (100, 70, 3, 44, 1, 1), (100, 70, 37, 65, 63, 5), (100, 80, 0, 60, 100, 20),
           (98, 72, 5, 1, 91, 3), (100, 70, 0, 90, 10, 10), (100, 70, 5, 5, 0, 9), (100, 70, 5, 5, 9, 0)]


@pytest.mark.parametrize("profile", [0, 1, 2, 3])
def test_plan_contents(built, profile):
    """FIXED, one k: `win` is t3hip_window_plan of one frame; one_launch = tile_range and tile_hi > tile_lo and n_frames >= 2 (so 0 for one
    frame, for a window wholly behind the stream, for an empty window, which plans no tile); byte counts, their stride minima rounded up
    to 16; scratch = n_frames runs at stride r16(6 * win.n_px) + the fixed slack on the one-launch path, the single-frame entry's own
    scratch on the loop path, nothing for an empty window."""
    t3 = built; k = SINGLE_K[profile]
    cfg = t3.make_cfg(profile=profile, uep=profile, mode=t3.MODE_FIXED)
    n_px = 7000; n_raw = n_px // 2
    words = t3.encoded_words(n_raw, cfg)
    assert -(-n_px // units_tile(k)) >= 3
    for win in WINDOWS:
        one = t3.window_plan(n_raw, cfg, *win)
        for fmt, ub in ((t3.WINDOW_PIXELS, 6), (t3.WINDOW_RGB, 3)):
            for n in (0, 1, 2, 3, 65535):
                p = t3.frames_window_plan(n_raw, n, cfg, *win, fmt)
                assert win_tuple(p.win) == win_tuple(one), (win, n)
                w, h = win[4], win[5]
                want_one = 1 if (one.tile_range == 1 and one.tile_hi > one.tile_lo and n >= 2 and w * h) else 0
                assert (p.n_frames, p.one_launch) == (n, want_one), (win, fmt, n)
                assert (p.in_bytes, p.out_bytes) == (9 * words, w * h * ub)
                assert (p.in_stride_min, p.out_stride_min) == (r16(9 * words), r16(w * h * ub))
                if w * h == 0:
                    assert (one.n_tiles, one.tile_lo, one.tile_hi) == (0, 0, 0) and p.scratch_bytes == 0
                elif want_one:
                    assert p.scratch_bytes == n * r16(6 * one.n_px) + SLACK
                elif n:
                    assert p.scratch_bytes == 6 * one.n_px + SLACK
                else:
                    assert p.scratch_bytes == 0
    behind = t3.frames_window_plan(n_raw, 3, cfg, 100, 70, 0, 90, 10, 10)
    assert behind.win.tile_range == 1 and behind.win.tile_lo == behind.win.tile_hi and behind.one_launch == 0
    # the 8K centre windows of the image front end: the plan of decode_images_async
    fw, fh = STD_RES[27]
    for sub in (24, 15):
        x0, y0, w, h = centered_window(sub)
        p = t3.frames_window_plan(fw * fh // 2, 4, cfg, fw, fh, x0, y0, w, h, t3.WINDOW_RGB)
        assert p.one_launch == 1 and p.out_bytes == 3 * w * h and p.scratch_bytes == 4 * r16(6 * p.win.n_px) + SLACK
        assert win_tuple(p.win) == win_tuple(t3.window_plan(fw * fh // 2, cfg, fw, fh, x0, y0, w, h))


def test_plan_per_frame_framings(built):
    """Per-band k, 2-D, beacon and COMPAT frames have no tile range: a loop of the single-frame entry, whose scratch is a whole frame."""
    t3 = built
    n_px = 7000; n_raw = n_px // 2
    others = [dict(profile=1, uep="luma", mode=1), dict(profile=4, uep=1, tile=(64, 64), mode=1), dict(profile=1, uep=1, beacon=(83, 2, 1), mode=1),
              dict(profile=2, uep=2, mode=0)]
    for kw in others:
        cfg = t3.make_cfg(**kw)
        for fmt in (t3.WINDOW_PIXELS, t3.WINDOW_RGB):
            p = t3.frames_window_plan(n_raw, 3, cfg, 100, 70, 10, 22, 50, 20, fmt)
            assert (p.one_launch, p.win.tile_range, p.win.n_tiles, p.n_frames) == (0, 0, 0, 3), kw
            assert p.scratch_bytes == 6 * n_px + SLACK and p.in_bytes == 9 * t3.encoded_words(n_raw, cfg)
            assert (p.in_stride_min, p.out_stride_min) == (r16(p.in_bytes), r16(p.out_bytes))


def test_plan_refusals(built):
    """RAW mode, x0 + w > fw, fw = 0, an output format other than 1 / 2, 65536 frames, 2^31 tickets or more, a null configuration: T3_E_ARG."""
    t3 = built
    cfg = t3.make_cfg(profile=2, uep=2, mode=t3.MODE_FIXED)
    n_raw = 3500
    bad = [
        dict(cfg=t3.make_cfg(profile=t3.ProfileID.RAW_MODE, mode=t3.MODE_FIXED)),
        dict(win=(100, 70, 98, 0, 3, 1)), dict(win=(0, 70, 0, 0, 0, 1)), dict(fmt=0), dict(fmt=3), dict(n=65536), dict(cfg=None),
    ]
    for kw in bad:
        with pytest.raises(t3.T3Error) as e:
            t3.frames_window_plan(n_raw, kw.get("n", 3), kw.get("cfg", cfg), *kw.get("win", (100, 70, 10, 22, 50, 20)), kw.get("fmt", t3.WINDOW_PIXELS))
        assert e.value.code == t3.E_ARG, kw
    assert t3.frames_window_plan(n_raw, 65535, cfg, 100, 70, 10, 22, 50, 20).one_launch == 1
    # tickets, as test_frames_plan.test_plan_limits builds them: 40,000 frames of 53,688 decoder tiles (k = 20: 52 blocks per band) are
    # 2^31 + 36,352 tickets, one tile less per frame stays below.  The frame is read as one row, the window is that row, so the range is
    # every tile; a window that leaves the first tile out is one tile per frame below again.
    for tiles, ok in ((53687, True), (53688, False)):
        n_px = 2 * (tiles * 52 * 20 * 9 * 3 // 26 - 40)
        assert -(-max(t3.plan(n_px // 2, cfg).band_blocks) // 52) == tiles
        if ok:
            p = t3.frames_window_plan(n_px // 2, 40000, cfg, n_px, 1, 0, 0, n_px, 1)
            assert p.one_launch == 1 and (p.win.tile_lo, p.win.tile_hi) == (0, tiles)
        else:
            with pytest.raises(t3.T3Error) as e:
                t3.frames_window_plan(n_px // 2, 40000, cfg, n_px, 1, 0, 0, n_px, 1)
            assert e.value.code == t3.E_ARG
            p = t3.frames_window_plan(n_px // 2, 40000, cfg, n_px, 1, 2160, 0, n_px - 2160, 1)
            assert p.one_launch == 1 and (p.win.tile_lo, p.win.tile_hi) == (1, tiles)
            assert t3.frames_window_plan(n_px // 2, 1, cfg, n_px, 1, 0, 0, n_px, 1).one_launch == 0


def test_entries_check_arguments_then_the_device(built):
    """The three batched device entries refuse what is wrong with their arguments before they ask for a device -- a null base of a batch
    that has bytes to move, a misaligned base, a stride that is no multiple of 16 or below the minimum, a missing verdict pointer:
    T3_E_ARG -- and only then answer T3_E_NODEVICE: no CPU fallback.  (The addresses are never read: no device, no launch.)"""
    t3 = built
    if t3.is_ready():
        pytest.skip("a context exists in this process")
    cfg = t3.make_cfg(profile=2, uep=2, mode=t3.MODE_FIXED)
    n = 3; n_raw = 3500; win = (100, 70, 10, 22, 50, 20)
    words = t3.encoded_words(n_raw, cfg)
    A, B, V = 1 << 20, 1 << 24, 1 << 28                        # three aligned addresses
    p = t3.frames_window_plan(n_raw, n, cfg, *win, t3.WINDOW_RGB)
    fw, fh, x0, y0, tw, th = t3.image_geometry(15, False)
    iw = t3.encoded_words(fw * fh // 2, cfg)
    ip = t3.frames_window_plan(fw * fh // 2, n, cfg, fw, fh, x0, y0, tw, th, t3.WINDOW_RGB)
    ep = t3.frames_plan(False, fw * fh, n, cfg, t3.FRAMES_RGB)
    sw, sh = 100, 75
    dec = lambda i, o, si=0, so=0, v=V, nf=n: t3.decode_frames_window_async(i, words, p.in_stride_min + si, nf, cfg, n_raw, *win, o, p.out_stride_min + so, t3.WINDOW_RGB, v)
    img = lambda i, o, si=0, so=0, v=V, nf=n: t3.decode_images_async(i, iw, ip.in_stride_min + si, nf, cfg, 15, False, o, ip.out_stride_min + so, v)
    enc = lambda i, o, si=0, so=0, v=V, nf=n: t3.encode_images_dev(i, sw, sh, sw * sh * 3 + si, nf, 15, False, cfg, o, ep.out_stride_min + so)
    bad = [dict(i=0, o=B), dict(i=A, o=0), dict(i=0, o=0), dict(i=A, o=B + 8), dict(i=A, o=B, so=8), dict(i=A, o=B, so=-16), dict(i=A, o=B, si=-16),
           dict(i=0, o=B, nf=1), dict(i=A, o=0, nf=1)]
    for fn in (dec, img, enc):
        both = bad + ([dict(i=A + 8, o=B), dict(i=A, o=B, si=8), dict(i=A, o=B, v=0), dict(i=A, o=B, v=0, nf=1)] if fn is not enc else [])
        for kw in both:
            with pytest.raises(t3.T3Error) as e:
                fn(**kw)
            assert e.value.code == t3.E_ARG, (fn is dec, fn is img, kw)
        for nf in (0, 1, n):
            with pytest.raises(t3.T3Error) as e:
                fn(i=A, o=B, nf=nf)
            assert e.value.code == t3.E_NODEVICE, (fn is dec, fn is img, nf)
    with pytest.raises(t3.T3Error) as e:                        # sources at any address: an odd one is well-formed
        enc(i=A + 5, o=B, si=5)
    assert e.value.code == t3.E_NODEVICE
    for kw in (dict(sub=16), dict(sw=65536)):                   # an invalid subword mode, a side >= 2^16
        with pytest.raises(t3.T3Error) as e:
            t3.encode_images_dev(A, kw.get("sw", sw), sh, 1 << 26, n, kw.get("sub", 15), False, cfg, B, ep.out_stride_min)
        assert e.value.code == t3.E_ARG, kw
    with pytest.raises(t3.T3Error) as e:
        t3.decode_images_async(A, iw, ip.in_stride_min, n, cfg, 16, False, B, ip.out_stride_min, V)
    assert e.value.code == t3.E_ARG
    # a per-frame framing (a beacon) and the window's own refusals are checked the same way
    bcn = t3.make_cfg(profile=1, uep=1, beacon=(83, 2, 1), mode=t3.MODE_FIXED)
    pb = t3.frames_window_plan(n_raw, n, bcn, *win)
    bw = t3.encoded_words(n_raw, bcn)
    for i, o in ((0, B), (A, 0), (A + 8, B)):
        with pytest.raises(t3.T3Error) as e:
            t3.decode_frames_window_async(i, bw, pb.in_stride_min, n, bcn, n_raw, *win, o, pb.out_stride_min, t3.WINDOW_PIXELS, V)
        assert e.value.code == t3.E_ARG
    with pytest.raises(t3.T3Error) as e:
        t3.decode_frames_window_async(A, words, p.in_stride_min, n, cfg, n_raw, 100, 70, 98, 0, 3, 1, B, p.out_stride_min, t3.WINDOW_RGB, V)
    assert e.value.code == t3.E_ARG
    with pytest.raises(t3.T3Error) as e:                        # the host entry: strides first, then the device
        t3.decode_frames_window([[[0] * 9] * words] * 2, cfg, n_raw, *win)
    assert e.value.code == t3.E_NODEVICE


NEW_KERNELS = ["window_crop_frames_kernel<false>", "window_crop_frames_kernel<true>", "image_compose_frames_kernel"]


def test_new_kernels_register_budget(built):
    """The batched crop (pixels / RGB out) and the batched compose are built, each once, spill no VGPR and use no scratch."""
    sys.path.insert(0, os.path.join(ROOT, "profiles"))
    import kernel_resources as kr
    ks = kr.all_kernels()
    for want in NEW_KERNELS:
        hit = [n for n in ks if want in n]
        assert len(hit) == 1, (want, hit)
        assert int(ks[hit[0]]["vgpr_spill_count"]) == 0 and int(ks[hit[0]]["sgpr_spill_count"]) == 0, (hit[0], ks[hit[0]])
        assert int(ks[hit[0]]["private_segment_fixed_size"]) == 0, (hit[0], ks[hit[0]])
