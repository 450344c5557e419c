"""Host-only part of the window decode with erasures (include/t3hip.h, "decode a window with erasures"):
t3hip_decode_erasures_window_plan over every configuration of tests/rs_patterns.py, both output formats and a handful of windows --
against t3hip_decode_erasures_plan, t3hip_window_plan and a numpy statement of the window definition --, the plan's refusals, the
refusals of the entries in a process that never initialised a device -- bad arguments, then a truncated stream, only then
T3_E_NODEVICE --, the exported symbols, and the register budget of decode_era_window_px<R, RGB, BCN>.  The GPU side is
tests/test_gpu_decode_erasures_window.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import rs_patterns as rp
from test_decode_erasures_plan import FUSED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("t3hip_decode_erasures_window_plan", "t3hip_decode_erasures_window_async", "t3hip_decode_erasures_window_dev", "t3hip_decode_erasures_window")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    return ge.load_package()


def test_symbols_exported(built):
    """The four entries are in the built library and the mirror has their wrappers; the plan's ctypes mirror has the C struct's size."""
    L = built.lib()
    for name in SYMBOLS:
        assert hasattr(L, name), name
    for name in ("decode_erasures_window_plan", "decode_erasures_window_async", "decode_erasures_window_dev", "decode_erasures_window", "DecodeErasuresWindowPlan"):
        assert callable(getattr(built, name)), name
    assert C.sizeof(built.WindowPlan) == 40 and C.sizeof(built.DecodeErasuresWindowPlan) == 72


def windows_of(n_px, k):
    """(fw, fh, x0, y0, w, h): a handful per frame size -- the full frame, one pixel, a window inside one tile, one the stream's end cuts,
    one past fh, one past the stream, one wholly behind it, one in a later tile only"""
    fw = 251; fh = -(-n_px // fw)
    out = [(fw, fh, 0, 0, fw, fh), (fw, fh, 17, 0, 1, 1), (fw, fh, 3, 1, 5, 2), (fw, fh, fw - 9, max(fh - 3, 0), 9, 3),
           (fw, max(fh - 1, 1), 0, 0, 8, fh), (fw, fh + 5, 1, 0, 3, fh + 4), (fw, fh + 40, 0, fh + 2, 4, 4), (7, -(-n_px // 7), 2, 1, 5, 3)]
    tile = 108 * k
    if n_px > 3 * tile:
        y = -(-2 * tile // fw)
        out.append((fw, fh, 100, y, 33, 2))                                 # behind tile 0 and tile 1
    return out


def needs_zero(n_px_stream, win):
    """numpy statement of the window definition: some window position is in a row >= fh or behind the stream"""
    fw, fh, x0, y0, w, h = win
    yy, xx = np.meshgrid(np.arange(h, dtype=np.int64), np.arange(w, dtype=np.int64), indexing="ij")
    s = (y0 + yy) * fw + x0 + xx
    return bool((((y0 + yy) >= fh) | (s >= n_px_stream)).any())


@pytest.mark.parametrize("n_px", (301, 2 * 108 * 24 * 3 + 7, 200_001))
@pytest.mark.parametrize("name", sorted(rp.CONFIGS))
def test_plan_per_configuration(built, name, n_px):
    """path = the erasure plan's; win = the window plan's, field for field; tiles_launched: the range, the frame's tiles with a beacon, 0 on
    path 0; zero_fill by the window definition; out_bytes; no scratch on path 1, the copy and the window entry's run on path 0."""
    t3 = built
    cfg = t3.make_cfg(mode=1, **rp.CONFIGS[name])
    n_raw = (n_px + 1) // 2
    L = t3.plan(n_raw, cfg)
    k = max(int(L.band_k[b]) for b in range(9))
    seen_range = seen_zero = seen_nozero = False
    for fmt in (1, 2):
        ep = t3.decode_erasures_plan(n_raw, cfg, fmt)
        assert ep.path == (1 if name in FUSED else 0)
        for win in windows_of(n_px, k):
            tag = (name, n_px, fmt, win)
            p = t3.decode_erasures_window_plan(n_raw, cfg, *win, fmt)
            wp = t3.window_plan(n_raw, cfg, *win)
            assert p.path == ep.path, tag
            for f, _ in t3.WindowPlan._fields_:
                if f != "pad_":
                    assert getattr(p.win, f) == getattr(wp, f), (tag, f)
            if p.path == 0:
                assert p.tiles_launched == 0 and wp.tile_range == 0, tag
                assert p.scratch_bytes == (9 * int(L.out_words) + 15) // 16 * 16 + 12 * n_raw + 256, tag
            else:
                assert p.scratch_bytes == 0, tag
                if name in rp.ONE_K:
                    assert wp.tile_range == 1 and p.tiles_launched == wp.tile_hi - wp.tile_lo, tag
                    seen_range |= 0 < p.tiles_launched < wp.n_tiles
                else:                                                       # a beacon: every tile of the frame
                    assert wp.tile_range == 0 and p.tiles_launched == ep.n_tiles > 0, tag
            assert p.zero_fill == (1 if needs_zero(2 * n_raw, win) else 0), tag
            seen_zero |= p.zero_fill == 1; seen_nozero |= p.zero_fill == 0
            assert p.in_bytes == 9 * int(L.out_words) and p.out_bytes == win[4] * win[5] * (6 if fmt == 1 else 3), tag
    assert seen_zero and seen_nozero
    if name in rp.ONE_K and n_px > 3 * 108 * k:
        assert seen_range, name


def test_no_window_pixel_in_the_stream(built):
    """A window wholly behind the stream on a tile range: no tile (the call does the header compare only and zeroes the window)."""
    t3 = built
    cfg = t3.make_cfg(mode=1, **rp.CONFIGS["k20"])
    p = t3.decode_erasures_window_plan(5000, cfg, 100, 400, 10, 300, 20, 20, 1)
    assert p.path == 1 and p.win.tile_range == 1 and p.win.tile_hi == p.win.tile_lo and p.tiles_launched == 0 and p.zero_fill == 1 and p.out_bytes == 2400


def test_plan_refusals(built):
    t3 = built; L = t3.lib()
    cfg = t3.make_cfg(profile=2, uep=2, mode=1)
    p = t3.DecodeErasuresWindowPlan()

    def plan(c=cfg, fw=100, x0=0, w=10, h=4, fmt=1, out=p, n_raw=640):
        return L.t3hip_decode_erasures_window_plan(C.c_uint64(n_raw), C.byref(c) if c is not None else None, C.c_uint32(fw), C.c_uint32(13), C.c_uint32(x0), C.c_uint32(1),
                                                   C.c_uint32(w), C.c_uint32(h), C.c_int(fmt), C.byref(out) if out is not None else None)
    assert plan() == t3.OK and p.path == 1 and p.out_bytes == 240
    assert plan(c=None) == t3.E_ARG and plan(out=None) == t3.E_ARG
    assert plan(fmt=0) == t3.E_ARG and plan(fmt=3) == t3.E_ARG
    assert plan(c=t3.make_cfg(profile=2, uep=2, mode=0)) == t3.E_ARG                   # COMPAT
    assert plan(c=t3.make_cfg(profile=0xFF, mode=1)) == t3.E_ARG                       # RAW mode
    assert plan(fw=0, w=0) == t3.E_ARG and plan(x0=91) == t3.E_ARG and plan(x0=90) == t3.OK
    assert plan(w=0) == t3.OK and p.out_bytes == 0 and p.tiles_launched == 0 and plan(h=0) == t3.OK and p.out_bytes == 0      # nothing to do is not an error
    assert plan(n_raw=0) == t3.OK and p.path == 0                                       # an empty frame: nothing for the fused kernel


NODEV = r"""
import ctypes as C, sys
sys.path.insert(0, %r)
import __graft_entry__ as ge
t3 = ge.load_package()
L = t3.lib()
assert not t3.is_ready()
cfg = t3.make_cfg(profile=2, uep=2, mode=1); compat = t3.make_cfg(profile=2, uep=2, mode=0); raw = t3.make_cfg(profile=0xFF, mode=1)
luma = t3.make_cfg(profile=1, uep="luma", mode=1)
n_raw = 64; n_in = int(t3.plan(n_raw, cfg).out_words); n_luma = int(t3.plan(n_raw, luma).out_words)
assert t3.decode_erasures_window_plan(n_raw, cfg, 16, 8, 2, 1, 9, 5, 1).path == 1 and t3.decode_erasures_window_plan(n_raw, luma, 16, 8, 2, 1, 9, 5, 1).path == 0
buf = (C.c_uint8 * (9 * max(n_in, n_luma) + 64))(); out = (C.c_uint8 * (6 * 9 * 5 + 64))(); ver = (C.c_uint32 * 4)(); cnt = (C.c_uint32 * 4)()
base = C.addressof(buf); base += -base %% 16
obase = C.addressof(out); obase += -obase %% 16
def run(i=base, n=n_in, c=cfg, fw=16, x0=2, w=9, h=5, o=obase, fmt=1, v=C.addressof(ver)):
    return L.t3hip_decode_erasures_window_async(C.c_void_p(i), C.c_uint64(n), C.byref(c) if c is not None else None, C.c_uint64(n_raw), C.c_uint32(fw), C.c_uint32(8),
                                                C.c_uint32(x0), C.c_uint32(1), C.c_uint32(w), C.c_uint32(h), C.c_void_p(o), C.c_int(fmt), C.c_void_p(v), None)
E_ARG, E_HEADER = t3.E_ARG, t3.E_HEADER
assert run(c=None) == E_ARG and run(v=None) == E_ARG and run(i=None) == E_ARG and run(i=base + 1) == E_ARG and run(o=None) == E_ARG
assert run(o=obase + 1) == E_ARG and run(o=obase + 2) == E_ARG                      # d_out: 4-byte aligned
assert run(fmt=0) == E_ARG and run(fmt=3) == E_ARG and run(c=compat) == E_ARG and run(c=raw) == E_ARG and run(fw=0) == E_ARG and run(x0=8) == E_ARG
assert run(n=n_in - 1) == E_HEADER and run(n=n_in - 1, fmt=2) == E_HEADER and run(n=n_luma - 1, c=luma) == E_HEADER    # path 1 and path 0 alike
assert run(n=n_in - 1, i=base + 1) == E_ARG and run(n=n_in - 1, o=obase + 2) == E_ARG and run(n=n_luma - 1, c=luma, x0=8) == E_ARG    # arguments first
assert run(w=0, o=None, i=None, n=0) == t3.OK and run(h=0) == t3.OK                 # nothing to do: no device asked for
assert run() == t3.E_NODEVICE and run(i=base + 2) == t3.E_NODEVICE and run(fmt=2, o=obase + 4) == t3.E_NODEVICE and run(n=n_luma, c=luma) == t3.E_NODEVICE
seen = t3.DecoderContext(mode=1).cfg_last_seen
def dev(i=base, s=seen, fw=16, x0=2, o=obase, fmt=1, c=cnt):
    return L.t3hip_decode_erasures_window_dev(C.c_void_p(i), C.c_uint64(n_in), C.byref(s) if s is not None else None, C.c_uint32(fw), C.c_uint32(8), C.c_uint32(x0),
                                              C.c_uint32(1), C.c_uint32(9), C.c_uint32(5), C.c_void_p(o), C.c_int(fmt), c, None)
def host(i=base, s=seen, fw=16, x0=2, o=obase, fmt=1, c=cnt):
    return L.t3hip_decode_erasures_window(C.c_void_p(i), C.c_uint64(n_in), C.byref(s) if s is not None else None, C.c_uint32(fw), C.c_uint32(8), C.c_uint32(x0),
                                          C.c_uint32(1), C.c_uint32(9), C.c_uint32(5), C.c_void_p(o), C.c_int(fmt), c)
for fn in (dev, host):
    assert fn(s=None) == E_ARG and fn(c=None) == E_ARG and fn(i=None) == E_ARG and fn(o=None) == E_ARG and fn(fmt=0) == E_ARG and fn(fmt=3) == E_ARG, fn.__name__
    assert fn(fw=0) == E_ARG and fn(x0=8) == E_ARG and fn(s=compat) == E_ARG and fn(s=raw) == E_ARG and fn() == t3.E_NODEVICE, fn.__name__
assert dev(i=base + 1) == E_ARG and dev(o=obase + 2) == E_ARG
assert all(x == 0 for x in ver) and all(x == 0 for x in cnt) and all(x == 0 for x in out)      # nothing was written anywhere
print("ok")
"""


def test_arguments_then_the_device(built):
    """A process that never initialised a device: bad arguments are refused before the entries ask for one, a truncated stream next (on a
    path-1 and on a path-0 configuration), and only then T3_E_NODEVICE (no CPU fallback).  (The addresses are host memory and never read:
    no device, no launch.)"""
    r = subprocess.run([sys.executable, "-c", NODEV % ROOT], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_kernel_register_budget(built):
    """decode_era_window_px<R, RGB, BCN> for the four codes, pixels and RGB, with and without beacon: built once each, no spilled VGPR, no
    scratch access inside the tile loop, 128 VGPRs at most (two 8-wave workgroups per CU, as decode_era_px_kernel)."""
    sys.path.insert(0, os.path.join(ROOT, "profiles"))
    import kernel_resources as kr
    ks = kr.all_kernels()
    loops = kr.loop_scratch(["t3_decode_era_window.o"])
    hits = [n for n in ks if "decode_era_window_px<" in n]
    assert len(hits) == 16, hits
    for n in hits:
        assert int(ks[n]["vgpr_spill_count"]) == 0 and int(ks[n]["vgpr_count"]) <= 128, (n, ks[n])
        assert loops[n] == (0, 0), (n, loops[n])
