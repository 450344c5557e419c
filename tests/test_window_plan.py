"""CPU-side checks of the window decode and the image front end (no GPU): the geometry of the five subword modes, the window plan
(which pixel tiles a window's rows live in), the integer form of resize_rgb_nn's index, and that the new compute entry points refuse
to run without a device.  Geometry and index maps are restated here in numpy from the reference's expressions
(old/include/ternary_image_codec_v6_min.hpp:117-146 std_res_for / centered_window, old/include/io_image.hpp:102-124)."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STD_RES = {27: (7680, 4320), 24: (3840, 2160), 21: (1920, 1080), 18: (1280, 720), 15: (854, 480)}    # std_res_for
PX_NB = 52                                                                                             # blocks per band of a pixel tile
SINGLE_K = {0: 24, 1: 22, 2: 20, 3: 18}                                                                # profile -> k, uep_uniform(profile)


def centered_window(sub):                                                                              # OLD:141-146
    fw, fh = STD_RES[27]; tw, th = STD_RES[sub]
    return (fw - tw) // 2, (fh - th) // 2, tw, th


def units_tile(k):
    return (9 * PX_NB * k // 13) * 3                                                                   # = 108 k pixels


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    return ge.load_package()


def test_image_geometry(built):
    for sub in (27, 24, 21, 18, 15):
        tw, th = STD_RES[sub]
        assert built.image_geometry(sub, False) == (tw, th, 0, 0, tw, th)
        if sub == 27:
            assert built.image_geometry(sub, True) == (tw, th, 0, 0, tw, th)
        else:
            x0, y0, w, h = centered_window(sub)
            assert built.image_geometry(sub, True) == (7680, 4320, x0, y0, w, h)
    for bad in (0, 26, 28, 12, -1, 255):
        with pytest.raises(built.T3Error) as e:
            built.image_geometry(bad, True)
        assert e.value.code == built.E_ARG


def check_range_plan(p, n_px, k, fw, fh, x0, y0, w, h):
    ut = units_tile(k)
    rows_end = min(y0 + h, fh)
    p0 = y0 * fw + x0
    p1 = min((rows_end - 1) * fw + x0 + w, n_px) if rows_end > y0 else 0
    assert p.tile_range == 1 and p.n_tiles == -(-n_px // ut)
    if p0 >= p1:
        assert p.tile_lo == p.tile_hi and p.n_px == 0
        return
    assert p.first_px == p.tile_lo * ut and p.first_px <= p0 and p1 <= p.first_px + p.n_px <= n_px
    assert p.n_px == min(p.tile_hi * ut, n_px) - p.first_px
    assert 0 < p.tile_hi - p.tile_lo <= -(-(p1 - p0) // ut) + 1, "the plan decodes more tiles than the window's rows touch"
    assert p.tile_hi <= p.n_tiles


def test_window_plan_8k_centred(built):
    fw, fh = STD_RES[27]; n_px = fw * fh; n_raw = n_px // 2
    share = {}
    for prof, k in SINGLE_K.items():
        cfg = built.make_cfg(profile=prof, uep=prof, mode=built.MODE_FIXED)
        for sub in (24, 21, 18, 15):
            x0, y0, w, h = centered_window(sub)
            p = built.window_plan(n_raw, cfg, fw, fh, x0, y0, w, h)
            check_range_plan(p, n_px, k, fw, fh, x0, y0, w, h)
            share[(k, sub)] = (p.tile_hi - p.tile_lo) / p.n_tiles
        # the first / last tile, full-width rows, the whole frame, a window running past fh
        for (x0, y0, w, h) in [(0, 0, 1, 1), (fw - 1, fh - 1, 1, 1), (0, 100, fw, 7), (0, 0, fw, fh), (3, 5, 11, 1), (100, fh - 10, 500, 50)]:
            check_range_plan(built.window_plan(n_raw, cfg, fw, fh, x0, y0, w, h), n_px, k, fw, fh, x0, y0, w, h)
        p = built.window_plan(n_raw, cfg, fw, fh, 0, 0, fw, fh)
        assert (p.tile_lo, p.tile_hi, p.first_px, p.n_px) == (0, p.n_tiles, 0, n_px)
        assert built.window_plan(n_raw, cfg, fw, fh, 0, 0, 1, 1).tile_hi == 1
        assert built.window_plan(n_raw, cfg, fw, fh, fw - 1, fh - 1, 1, 1).tile_lo == p.n_tiles - 1
    for (k, sub), s in share.items():                                    # the share of the frame the window's rows span, within two tiles
        tw, th = STD_RES[sub]
        span, nt = ((th - 1) * fw + tw) / units_tile(k), -(-n_px // units_tile(k))
        assert span <= s * nt <= span + 2, (k, sub, s)
        assert abs(s - th / fh) < 0.001, (k, sub, s)                     # S24 0.500, S21 0.250, S18 0.167, S15 0.111


def test_window_plan_edges_and_refusals(built):
    cfg = built.make_cfg(profile=2, uep=2, mode=built.MODE_FIXED)
    fw, fh = 960, 540; n_px = fw * fh; n_raw = n_px // 2
    # a window wholly behind the stream / below fh: nothing to decode
    for (x0, y0, w, h) in [(0, fh, 10, 10), (5, fh + 7, 3, 1)]:
        p = built.window_plan(n_raw, cfg, fw, fh, x0, y0, w, h)
        assert p.tile_range == 1 and p.tile_lo == p.tile_hi and p.n_px == 0
    p = built.window_plan(n_raw // 2, cfg, fw, fh, 0, fh // 2 + 1, fw, 10)            # fw * fh larger than the stream
    assert p.tile_range == 1 and p.tile_lo == p.tile_hi and p.n_px == 0
    check_range_plan(built.window_plan(n_raw // 2, cfg, fw, fh, 0, fh // 2 - 3, fw, 10), n_px // 2, 20, fw, fh, 0, fh // 2 - 3, fw, 10)
    # an empty window: T3_OK and an all-zero plan
    for (w, h) in [(0, 5), (5, 0), (0, 0)]:
        p = built.window_plan(n_raw, cfg, fw, fh, 0, 0, w, h)
        assert (p.tile_range, p.n_tiles, p.tile_lo, p.tile_hi, p.n_px) == (0, 0, 0, 0, 0), (w, h)
    for args in [(fw, fh, fw - 3, 0, 4, 1), (0, fh, 0, 0, 0, 1), (fw, fh, 0xFFFFFFFF, 0, 2, 1)]:
        with pytest.raises(built.T3Error) as e:
            built.window_plan(n_raw, cfg, *args)
        assert e.value.code == built.E_ARG, args
    with pytest.raises(built.T3Error) as e:
        built.window_plan(n_raw, built.make_cfg(profile=built.ProfileID.RAW_MODE, mode=built.MODE_FIXED), fw, fh, 0, 0, 4, 4)
    assert e.value.code == built.E_ARG
    # framings without a tile range: the whole frame
    others = [dict(profile=1, uep="luma"), dict(profile=4, uep=2, tile=(64, 64)), dict(profile=4, uep="luma", tile=(64, 64)),
              dict(profile=1, uep=1, beacon=(83, 2, 1))]
    for kw in others:
        p = built.window_plan(n_raw, built.make_cfg(mode=built.MODE_FIXED, **kw), fw, fh, 10, 10, 100, 100)
        assert (p.tile_range, p.n_tiles, p.tile_lo, p.tile_hi, p.first_px, p.n_px) == (0, 0, 0, 0, 0, n_px), kw
    p = built.window_plan(n_raw, built.make_cfg(profile=2, uep=2, mode=built.MODE_COMPAT), fw, fh, 10, 10, 100, 100)
    assert p.tile_range == 0 and p.n_px == n_px
    # P5 without a tile is 1-D: a tile range again
    assert built.window_plan(n_raw, built.make_cfg(profile=4, uep=1, mode=built.MODE_FIXED), fw, fh, 10, 10, 100, 100).tile_range == 1


def test_resize_index_integer_form():
    """resize_rgb_nn's index, (int)((x + 0.5) * (double)sw / dw) clamped to [0, sw - 1] (io_image.hpp:111-116), equals
    floor((2 x + 1) sw / (2 dw)) for sides below 2^16 and the clamp never acts: the exact quotient, when it is not an integer, is at
    least 1 / (2 dw) >= 2^-17 away from the next one, the double expression's rounding error is below 2^-36."""
    rng = np.random.default_rng(7)
    sides = [1, 2, 3, 5, 480, 854, 1080, 1920, 4320, 7680, 65535]
    pairs = [(a, b) for a in sides for b in sides] + [tuple(int(v) for v in rng.integers(1, 65536, 2)) for _ in range(40)]
    for sw, dw in pairs:
        x = np.arange(dw, dtype=np.int64)
        ref = ((x.astype(np.float64) + 0.5) * np.float64(sw) / np.float64(dw)).astype(np.int64)          # C's (int): truncation, values >= 0
        integer = (2 * x + 1) * sw // (2 * dw)
        assert np.array_equal(ref, integer), (sw, dw)
        assert integer.min() >= 0 and integer.max() <= sw - 1, (sw, dw)


NODEV = r"""
import ctypes as C, sys
sys.path.insert(0, %r)
import __graft_entry__ as ge
t3 = ge.load_package()
L = t3.lib()
assert not t3.is_ready()
cfg = t3.make_cfg(profile=2, uep=2, mode=1)
buf = (C.c_uint8 * 4096)(); ver = (C.c_uint32 * 2)(); n = C.c_uint64()
vp = C.cast(buf, C.c_void_p)
rcs = dict(
    window=L.t3hip_decode_window_async(vp, C.c_uint64(100), C.byref(cfg), C.c_uint64(64), C.c_uint32(16), C.c_uint32(8), C.c_uint32(0), C.c_uint32(0),
                                       C.c_uint32(4), C.c_uint32(4), vp, C.c_int(2), C.cast(ver, C.c_void_p), None),
    resize_dev=L.t3hip_resize_rgb_nn_dev(vp, 4, 4, vp, 8, 8, None),
    resize=L.t3hip_resize_rgb_nn(vp, 4, 4, vp, 8, 8),
    compose_dev=L.t3hip_image_compose_dev(vp, 4, 4, 15, 0, vp, None),
    compose=L.t3hip_image_compose(vp, 4, 4, 15, 0, vp),
    encode_image=L.t3hip_encode_image_dev(vp, 4, 4, 15, 0, C.byref(cfg), vp, C.c_uint64(1), C.byref(n), None),
    decode_image=L.t3hip_decode_image_async(vp, C.c_uint64(100), C.byref(cfg), 15, 0, vp, C.cast(ver, C.c_void_p), None))
bad = {k: v for k, v in rcs.items() if v != t3.E_NODEVICE}
assert not bad, bad
# the host-only calls still work
assert t3.image_geometry(15, True) == (7680, 4320, 3413, 1920, 854, 480)
assert t3.window_plan(64, cfg, 16, 8, 0, 0, 4, 4).tile_range == 1
print("ok")
"""


def test_new_entries_need_a_device(built):
    """A process that never initialised a device: every new compute entry answers T3_E_NODEVICE (no CPU fallback), the plan and the
    geometry answer."""
    r = subprocess.run([sys.executable, "-c", NODEV % ROOT], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def build_image_demo(tmp):
    exe = os.path.join(tmp, "image_names_demo")
    lib = os.path.join(ROOT, "ternary-image-codec_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "image_names_demo.cpp"),
                    "-L" + lib, "-lt3hip", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-o", exe], check=True)
    return exe


def test_image_names_demo_host_part(built, tmp_path):
    """tests/cpp/image_names_demo.cpp compiles against include/ternary_codec_v6.hpp; its host part (pad_even, the geometry next to the
    header's std_res_for / centered_window) runs without a device."""
    exe = build_image_demo(str(tmp_path))
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines()
    assert out[0] == "pad_even 0 2 7680 854"
    assert len(out) == 11
    for line in out[1:]:
        f = line.split()
        sub, centered = int(f[1]), int(f[2])
        g = tuple(int(v) for v in f[4:10]); std = (int(f[11]), int(f[12])); win = (int(f[14]), int(f[15]))
        assert f[3] == "rc=0" and std == STD_RES[sub] and g[4:] == std
        assert win == centered_window(sub)[:2]
        assert g[:4] == ((7680, 4320) + win if centered and sub != 27 else std + (0, 0))
