"""CPU-side checks of the batch entries (N equal frames in one call, include/t3hip.h; no GPU): the plan -- tiles per frame, the
bytes and minimum strides of one frame, which framings run as one launch -- the argument limits, that the compute entries refuse to
run without a device, and the register budget of the batch kernels read from the built objects."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SINGLE_K = {0: 24, 1: 22, 2: 20, 3: 18}            # profile -> k with uep_uniform(profile)
UNIT = {0: 9, 1: 6, 2: 3}                          # bytes of a raw word, a pixel record, an RGB pixel


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    return ge.load_package()


def r16(x):
    return (x + 15) & ~15


def cfg_of(t3, profile=2, mode=1, **kw):
    return t3.make_cfg(profile=profile, uep=kw.pop("uep", profile if profile < 4 else 1), mode=mode, **kw)


SIZES = [4861, 100, 854 * 480, 1920 * 1080]
# blocks per band of an encoder tile, (k, unit format): pixels 1 / RGB 2
ENC_NB = {(24, 1): 46, (24, 2): 56, (22, 1): 49, (22, 2): 49, (20, 1): 55, (20, 2): 55, (18, 1): 56, (18, 2): 56}


@pytest.mark.parametrize("profile", [0, 1, 2, 3])
def test_plan_tiles_and_strides(built, profile):
    """Tiles per frame, bytes and stride minima, and which direction runs as one launch, for the four codes.
    Decode: a pixel tile of the fused decoder is 52 blocks per band = 9 * 52 * k stream symbols = 108 k pixels, so tiles_per_frame ==
    ceil(n_px / (108 k)) (the pad pixel of an odd frame is coded too).  Encode: the fused encoder's tile is NOT 52 blocks per band: it is
    ENC_NB blocks per band, picked per code and front end by the encode planner's cost model under its limits (8 waves = 512 lanes dealt
    to 9 nb blocks, so nb <= 56; three workgroups' LDS), the same in both modes and for every frame size -- so tiles_per_frame ==
    ceil(max band blocks / ENC_NB[k, front end]).
    A frame's bytes are its units and its coded words (t3hip_plan), the stride minima those rounded up to 16."""
    t3 = built; k = SINGLE_K[profile]
    for mode in (t3.MODE_COMPAT, t3.MODE_FIXED):
        cfg = cfg_of(t3, profile, mode)
        for fmt in (t3.FRAMES_PIXELS, t3.FRAMES_RGB):
            nb = ENC_NB[k, fmt]
            for n_px in SIZES:
                n_raw = (n_px + 1) // 2
                words = t3.encoded_words(n_raw, cfg); maxb = max(t3.plan(n_raw, cfg).band_blocks)
                e = t3.frames_plan(False, n_px, 3, cfg, fmt)
                assert (e.n_frames, e.one_launch) == (3, 1), (mode, fmt, n_px)
                assert e.tiles_per_frame == -(-maxb // nb), (k, mode, fmt, n_px, maxb, e.tiles_per_frame)
                assert (e.in_bytes, e.out_bytes) == (n_px * UNIT[fmt], 9 * words)
                assert (e.in_stride_min, e.out_stride_min) == (r16(e.in_bytes), r16(e.out_bytes))
                d = t3.frames_plan(True, n_px, 3, cfg, fmt)
                assert d.one_launch == (1 if mode == t3.MODE_FIXED else 0), (mode, fmt, n_px)    # COMPAT decode: the per-frame path
                assert d.tiles_per_frame == (-(-2 * n_raw // (108 * k)) if mode == t3.MODE_FIXED else 0), (mode, fmt, n_px)
                assert (d.in_bytes, d.out_bytes) == (9 * words, 2 * n_raw * UNIT[fmt])
                assert (d.in_stride_min, d.out_stride_min) == (r16(d.in_bytes), r16(d.out_bytes))


def test_plan_per_frame_framings(built):
    """Everything the fused single-k kernels do not serve is a loop of the single-frame path: raw words, per-band k, 2-D, beacon, one
    frame, no words."""
    t3 = built
    fixed = cfg_of(t3, 2, t3.MODE_FIXED)
    per_frame = [
        (t3.FRAMES_WORDS, 2431, 3, fixed),                                                        # raw words either way
        (t3.FRAMES_PIXELS, 4861, 3, t3.make_cfg(profile=1, uep="luma", mode=t3.MODE_FIXED)),     # luma UEP: per-band k
        (t3.FRAMES_PIXELS, 4861, 3, t3.make_cfg(profile=4, uep=1, tile=(64, 64), mode=t3.MODE_FIXED)),   # P5 with a tile: 2-D
        (t3.FRAMES_PIXELS, 4861, 3, t3.make_cfg(profile=1, uep=1, beacon=(83, 2, 1), mode=t3.MODE_FIXED)),   # beacon
        (t3.FRAMES_PIXELS, 4861, 1, fixed),                                                       # one frame: the single-frame entry
        (t3.FRAMES_PIXELS, 0, 3, fixed),                                                          # no raw words
        (t3.FRAMES_RGB, 4861, 3, t3.make_cfg(profile=1, uep="luma", mode=t3.MODE_FIXED)),
    ]
    for fmt, n_units, n_frames, cfg in per_frame:
        for decode in (False, True):
            p = t3.frames_plan(decode, n_units, n_frames, cfg, fmt)
            assert (p.one_launch, p.tiles_per_frame, p.n_frames) == (0, 0, n_frames), (fmt, n_units, n_frames, decode)
            assert (p.in_stride_min, p.out_stride_min) == (r16(p.in_bytes), r16(p.out_bytes))
    w = t3.frames_plan(False, 2431, 3, fixed, t3.FRAMES_WORDS)
    assert (w.in_bytes, w.out_bytes) == (2431 * 9, 9 * t3.encoded_words(2431, fixed))
    assert t3.frames_plan(False, 4861, 0, fixed).n_frames == 0                                    # the empty batch plans


def test_plan_limits(built):
    """More than 65535 frames, 2^31 tickets or more, a null configuration or an unknown format: T3_E_ARG."""
    t3 = built
    cfg = cfg_of(t3, 2, t3.MODE_FIXED)
    assert t3.frames_plan(False, 2160, 65535, cfg).one_launch == 1
    for decode in (False, True):
        with pytest.raises(t3.T3Error) as e:
            t3.frames_plan(decode, 2160, 65536, cfg)
        assert e.value.code == t3.E_ARG
        # 40,000 frames of 53,688 tiles = 2^31 + 36,352 tickets; one tile less per frame stays below and plans.  k = 20: a tile is nb
        # blocks per band, nb = 52 (decoder) / 55 (encoder, pixels), and a band of a frame of W words has ceil(26 W / 3 / 9 / 20) blocks
        nb = 52 if decode else 55
        for tiles, ok in ((53687, True), (53688, False)):
            n_px = 2 * (tiles * nb * 20 * 9 * 3 // 26 - 40)                                      # a little under `tiles` full tiles
            assert -(-max(t3.plan(n_px // 2, cfg).band_blocks) // nb) == tiles
            if ok:
                assert t3.frames_plan(decode, n_px, 40000, cfg).tiles_per_frame == tiles
            else:
                with pytest.raises(t3.T3Error) as e:
                    t3.frames_plan(decode, n_px, 40000, cfg)
                assert e.value.code == t3.E_ARG
        with pytest.raises(t3.T3Error) as e:
            t3.frames_plan(decode, 2160, 3, None)
        assert e.value.code == t3.E_ARG
        with pytest.raises(t3.T3Error) as e:
            t3.frames_plan(decode, 2160, 3, cfg, 3)
        assert e.value.code == t3.E_ARG


def test_entries_check_arguments_then_the_device(built):
    """The batch device entries refuse what is wrong with their arguments before they ask for a device -- a null base of a batch that has
    bytes to move (0 is 16-byte aligned: it must never reach a launch), a misaligned base, a stride that is no multiple of 16 or below the
    plan's minimum: T3_E_ARG -- and only then T3_E_NODEVICE: no CPU fallback.  (The addresses are never read: no device, no launch.)"""
    t3 = built
    if t3.is_ready():
        pytest.skip("a context exists in this process")
    cfg = cfg_of(t3, 2, t3.MODE_FIXED)
    n, n_px = 2, 2160
    e_, d_ = t3.frames_plan(False, n_px, n, cfg), t3.frames_plan(True, n_px, n, cfg)
    words = e_.out_bytes // 9
    A, B = 1 << 20, 1 << 24                                     # two aligned addresses
    enc = lambda i, o, si=0, so=0, nf=n: t3.encode_frames_dev(i, n_px, t3.FRAMES_PIXELS, e_.in_stride_min + si, nf, cfg, o, e_.out_stride_min + so)
    dec = lambda i, o, si=0, so=0, v=A, nf=n: t3.decode_frames_async(i, words, d_.in_stride_min + si, nf, cfg, n_px // 2, o, d_.out_stride_min + so, t3.FRAMES_PIXELS, v)
    bad = [dict(i=0, o=B), dict(i=A, o=0), dict(i=0, o=0), dict(i=A + 8, o=B), dict(i=A, o=B + 8), dict(i=A, o=B, si=8), dict(i=A, o=B, so=8),
           dict(i=A, o=B, si=-16), dict(i=A, o=B, so=-16), dict(i=0, o=B, nf=1), dict(i=A, o=0, nf=1)]
    for fn in (enc, dec):
        for kw in bad:
            with pytest.raises(t3.T3Error) as e:
                fn(**kw)
            assert e.value.code == t3.E_ARG, (fn is enc, kw)
        for nf in (0, 1, n):
            with pytest.raises(t3.T3Error) as e:
                fn(i=A, o=B, nf=nf)
            assert e.value.code == t3.E_NODEVICE, (fn is enc, nf)
    with pytest.raises(t3.T3Error) as e:
        dec(i=A, o=B, v=0)                                      # no verdict words
    assert e.value.code == t3.E_ARG
    # per-frame framings (a beacon) are checked the same way
    bcn = t3.make_cfg(profile=1, uep=1, beacon=(83, 2, 1), mode=t3.MODE_FIXED)
    pb = t3.frames_plan(False, n_px, n, bcn)
    for i, o in ((0, B), (A, 0)):
        with pytest.raises(t3.T3Error) as e:
            t3.encode_frames_dev(i, n_px, t3.FRAMES_PIXELS, pb.in_stride_min, n, bcn, o, pb.out_stride_min)
        assert e.value.code == t3.E_ARG
    with pytest.raises(t3.T3Error) as e:
        t3.encode_frames([np.zeros(100, t3.PIXEL_DT)] * 2, cfg)
    assert e.value.code == t3.E_NODEVICE


BATCH_KERNELS = ["enc_frames_k<%d, %d>" % (fe, r) for fe in (0, 2) for r in (2, 4, 6, 8)] + \
                ["dec_frames_px<%d, %s, false>" % (r, rgb) for r in (2, 4, 6, 8) for rgb in ("false", "true")]


def test_batch_kernels_register_budget(built):
    """The 16 batch kernels -- enc_frames_k<front end, r>: pixels / RGB x four codes; dec_frames_px<r, RGB, no beacon> -- are built,
    each once, carry no spilled VGPR and touch no scratch inside their tile loop (as test_no_vgpr_spills_in_hot_kernels asks of their
    single-frame twins encode_kernel_k<fe, 0, r, false> and decode_fixed_px_kernel<r, rgb, false>, none of which spills)."""
    sys.path.insert(0, os.path.join(ROOT, "profiles"))
    import kernel_resources as kr
    ks = kr.all_kernels()
    loops = kr.loop_scratch(["t3_encode_frames.o", "t3_decode_frames.o"])
    assert sorted(n for n in ks if "enc_frames_k" in n or "dec_frames_px" in n) == sorted(loops), "a batch kernel without a tile loop"
    for want in BATCH_KERNELS:
        hit = [n for n in ks if want in n]
        assert len(hit) == 1, (want, hit)
        assert int(ks[hit[0]]["vgpr_spill_count"]) == 0, (hit[0], ks[hit[0]])
        assert loops[hit[0]] == (0, 0), (hit[0], loops[hit[0]])
    assert len(loops) == len(BATCH_KERNELS)
    # the names leave the single-frame kernels' name tests alone (tests/test_host_logic.py matches by substring)
    assert not any("encode_kernel_" in n or "decode_fixed_px_kernel" in n for n in loops)
