"""Host-only part of the window decode with erasures over a batch of equal frames (include/t3hip.h, "decode a window with erasures of a
batch of equal FIXED frames"): t3hip_decode_erasures_frames_window_plan over every configuration of tests/rs_patterns.py, both output
formats, a handful of windows and four batch sizes -- against t3hip_decode_erasures_window_plan and the rules of the header comment --,
the plan's refusals, the refusals of the three entries in a process that never initialised a device -- bad arguments, then a truncated
stream, only then T3_E_NODEVICE --, the exported symbols, the register budget of decode_era_frames_window_px<R, RGB, BCN>, and the masking
conditions of the GPU tests (tests/test_gpu_decode_erasures_frames_window.py), proved here with the yardstick alone."""
import ctypes as C
import os
import subprocess
import sys

import pytest

import rs_patterns as rp
from test_decode_erasures_plan import FUSED
from test_decode_erasures_window_plan import windows_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("t3hip_decode_erasures_frames_window_plan", "t3hip_decode_erasures_frames_window_async", "t3hip_decode_erasures_frames_window_dev",
           "t3hip_decode_erasures_frames_window")
MAX_FRAMES = 65535                                                        # kRepairMaxFrames


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    return ge.load_package()


def test_symbols_exported(built):
    """The four entries are in the built library, the mirror has their wrappers, and the ctypes struct has the C struct's size: the
    single-frame window plan (72 bytes), n_frames, one_launch and padding, tiles_launched and padding (16), four 64-bit fields; the C side
    writes exactly that many bytes."""
    L = built.lib()
    for name in SYMBOLS:
        assert hasattr(L, name), name
    for name in ("DecodeErasuresFramesWindowPlan", "decode_erasures_frames_window_plan", "decode_erasures_frames_window_async", "decode_erasures_frames_window_dev",
                 "decode_erasures_frames_window"):
        assert callable(getattr(built, name)), name
    assert C.sizeof(built.DecodeErasuresFramesWindowPlan) == C.sizeof(built.DecodeErasuresWindowPlan) + 16 + 4 * 8 == 120

    class Guarded(C.Structure):
        _fields_ = [("p", built.DecodeErasuresFramesWindowPlan), ("guard", C.c_uint8 * 64)]
    g = Guarded(); C.memset(C.byref(g), 0xA5, C.sizeof(g))
    cfg = built.make_cfg(mode=1, **rp.CONFIGS["k20"])
    assert L.t3hip_decode_erasures_frames_window_plan(C.c_uint64(5000), C.c_uint32(5), C.byref(cfg), C.c_uint32(100), C.c_uint32(100), C.c_uint32(3), C.c_uint32(30),
                                                      C.c_uint32(11), C.c_uint32(7), C.c_int(2), C.byref(g.p)) == built.OK
    assert bytes(g.guard) == b"\xA5" * 64 and g.p.n_frames == 5 and g.p.one_launch == 1 and g.p.out_bytes == 231 and g.p.out_stride_min == 240
    assert list(g.p.pad_) == [0, 0, 0] and g.p.pad2_ == 0 and g.p.tiles_launched == 5 * g.p.frame.tiles_launched > 0
    import numpy as np
    assert built.decode_erasures_frames_window(np.zeros((0, 18), "uint8"), built.DecoderContext(mode=1), 4, 4, 0, 0, 2, 2, 1) == (built.OK, [], [], [])


@pytest.mark.parametrize("n_px", (301, 2 * 108 * 24 * 3 + 7, 200_001))
@pytest.mark.parametrize("name", sorted(rp.CONFIGS))
def test_plan_per_configuration(built, name, n_px):
    """`frame` is t3hip_decode_erasures_window_plan's struct, byte for byte and field for field; one_launch exactly where that plan says
    path 1 with at least one tile and the batch has two frames at least; tiles_launched the batch's tickets; the input stride minimum the
    frame's bytes rounded up to even, the output's the window's bytes rounded up to 16; the one-launch path holds no scratch, the loop one
    frame's.  A window wholly behind the stream on a one-k framing has no tile: the loop."""
    t3 = built
    cfg = t3.make_cfg(mode=1, **rp.CONFIGS[name])
    n_raw = (n_px + 1) // 2
    L = t3.plan(n_raw, cfg)
    k = max(int(L.band_k[b]) for b in range(9))
    seen_one = seen_behind = False
    for fmt in (1, 2):
        for win in windows_of(n_px, k):
            single = t3.decode_erasures_window_plan(n_raw, cfg, *win, fmt)
            for n_frames in (0, 1, 2, 3):
                tag = (name, n_px, fmt, win, n_frames)
                p = t3.decode_erasures_frames_window_plan(n_raw, n_frames, cfg, *win, fmt)
                assert bytes(p.frame) == bytes(single) and p.n_frames == n_frames, tag
                for f, _ in t3.DecodeErasuresWindowPlan._fields_:
                    if f not in ("pad_", "win"):
                        assert getattr(p.frame, f) == getattr(single, f), (tag, f)
                for f, _ in t3.WindowPlan._fields_:
                    if f != "pad_":
                        assert getattr(p.frame.win, f) == getattr(single.win, f), (tag, f)
                one = 1 if single.path == 1 and n_frames >= 2 and single.tiles_launched > 0 else 0
                assert p.one_launch == one and p.tiles_launched == (n_frames * single.tiles_launched if one else 0), tag
                assert p.in_stride_min == single.in_bytes + single.in_bytes % 2 == 9 * int(L.out_words) + (9 * int(L.out_words)) % 2, tag
                assert p.out_bytes == win[4] * win[5] * (6 if fmt == 1 else 3) and p.out_stride_min == (p.out_bytes + 15) // 16 * 16, tag
                assert p.scratch_bytes == (0 if one else single.scratch_bytes), tag
                assert single.path == (1 if name in FUSED else 0) and (one == 0 or name in FUSED), tag
                seen_one |= one == 1
                if name in rp.ONE_K and single.win.tile_hi == single.win.tile_lo:          # no window position is in the stream
                    assert single.tiles_launched == 0 and p.one_launch == 0 and p.scratch_bytes == 0, tag
                    seen_behind |= n_frames >= 2
    assert seen_one == (name in FUSED) and seen_behind == (name in rp.ONE_K)


def test_plan_refusals(built):
    t3 = built; L = t3.lib()
    cfg = t3.make_cfg(profile=2, uep=2, mode=1)
    p = t3.DecodeErasuresFramesWindowPlan()

    def plan(c=cfg, n=5, fw=100, fh=13, x0=0, y0=1, w=10, h=4, fmt=1, out=p, n_raw=640):
        return L.t3hip_decode_erasures_frames_window_plan(C.c_uint64(n_raw), C.c_uint32(n), C.byref(c) if c is not None else None, C.c_uint32(fw), C.c_uint32(fh), C.c_uint32(x0),
                                                          C.c_uint32(y0), C.c_uint32(w), C.c_uint32(h), C.c_int(fmt), C.byref(out) if out is not None else None)
    assert plan() == t3.OK and p.one_launch == 1 and p.frame.path == 1 and p.out_bytes == 240 and p.n_frames == 5
    assert plan(c=None) == t3.E_ARG and plan(out=None) == t3.E_ARG
    assert plan(fmt=0) == t3.E_ARG and plan(fmt=3) == t3.E_ARG
    assert plan(c=t3.make_cfg(profile=2, uep=2, mode=0)) == t3.E_ARG                   # COMPAT
    assert plan(c=t3.make_cfg(profile=0xFF, mode=1)) == t3.E_ARG                       # RAW mode
    assert plan(fw=0, w=0) == t3.E_ARG and plan(x0=91) == t3.E_ARG and plan(x0=90) == t3.OK
    assert plan(n=MAX_FRAMES) == t3.OK and plan(n=MAX_FRAMES + 1) == t3.E_ARG and plan(n=MAX_FRAMES + 1, c=t3.make_cfg(profile=1, uep="luma", mode=1)) == t3.E_ARG
    assert plan(n=0) == t3.OK and p.one_launch == 0 and p.n_frames == 0 and p.tiles_launched == 0
    for kw in (dict(w=0), dict(h=0)):                                                   # nothing to do is not an error
        assert plan(**kw) == t3.OK and p.out_bytes == 0 and p.one_launch == 0 and p.tiles_launched == 0 and p.out_stride_min == 0, kw
    assert plan(n_raw=0) == t3.OK and p.frame.path == 0 and p.one_launch == 0           # empty frames: nothing for the fused kernel
    # the one launch's ticket space is 32-bit: a k20 pixel tile holds 2160 pixels; rows of one tile each
    n_raw = 32768 * 1080
    whole = dict(fw=2160, fh=32769, y0=0, w=2160)
    assert plan(n=MAX_FRAMES, n_raw=n_raw, h=32768, **whole) == t3.OK and p.frame.tiles_launched == 32768 and p.tiles_launched == MAX_FRAMES * 32768 < 2 ** 31
    assert plan(n=MAX_FRAMES, n_raw=n_raw + 1080, h=32769, **whole) == t3.E_ARG and MAX_FRAMES * 32769 >= 2 ** 31
    assert plan(n=MAX_FRAMES, n_raw=n_raw + 1080, h=32768, **whole) == t3.OK            # the same frames, a window of one tile less
    assert plan(n=1, n_raw=n_raw + 1080, h=32769, **whole) == t3.OK and p.one_launch == 0      # the loop has no such bound
    assert plan(n=MAX_FRAMES, n_raw=n_raw + 1080, h=32769, c=t3.make_cfg(profile=1, uep="luma", mode=1), **whole) == t3.OK and p.one_launch == 0


NODEV = r"""
import ctypes as C, sys
sys.path.insert(0, %r)
import __graft_entry__ as ge
t3 = ge.load_package()
L = t3.lib()
assert not t3.is_ready()
cfg = t3.make_cfg(profile=2, uep=2, mode=1); compat = t3.make_cfg(profile=2, uep=2, mode=0); raw = t3.make_cfg(profile=0xFF, mode=1)
luma = t3.make_cfg(profile=1, uep="luma", mode=1)
n_raw = 64; n_in = int(t3.plan(n_raw, cfg).out_words); n_luma = int(t3.plan(n_raw, luma).out_words); N = 3
WIN = (16, 8, 2, 1, 9, 5)
p = t3.decode_erasures_frames_window_plan(n_raw, N, cfg, *WIN, 1); q = t3.decode_erasures_frames_window_plan(n_raw, N, luma, *WIN, 1)
assert p.one_launch == 1 and q.one_launch == 0 and p.frame.path == 1 and q.frame.path == 0
stride = p.in_stride_min; st_luma = q.in_stride_min; ostride = p.out_stride_min
assert stride == 9 * n_in + (9 * n_in & 1) and p.out_bytes == 270 and ostride == 272
buf = (C.c_uint8 * (N * max(stride, st_luma) + 64))(); out = (C.c_uint8 * (N * (ostride + 16) + 64))(); ver = (C.c_uint32 * (4 * N))(); cnt = (C.c_uint32 * (4 * N))()
rcs = (C.c_int * N)()
base = C.addressof(buf); base += -base %% 16
obase = C.addressof(out); obase += -obase %% 16
E_ARG, E_HEADER, NODEV, OK = t3.E_ARG, t3.E_HEADER, t3.E_NODEVICE, t3.OK
def run(i=base, n=n_in, st=stride, nf=N, c=cfg, fw=16, x0=2, w=9, h=5, o=obase, ost=ostride, fmt=1, v=C.addressof(ver)):
    return L.t3hip_decode_erasures_frames_window_async(C.c_void_p(i), C.c_uint64(n), C.c_uint64(st), C.c_uint32(nf), C.byref(c) if c is not None else None, C.c_uint64(n_raw),
                                                       C.c_uint32(fw), C.c_uint32(8), C.c_uint32(x0), C.c_uint32(1), C.c_uint32(w), C.c_uint32(h), C.c_void_p(o), C.c_uint64(ost),
                                                       C.c_int(fmt), C.c_void_p(v), None)
# every class of bad argument, on the path-1 and on the path-0 configuration
for c, n, st in ((cfg, n_in, stride), (luma, n_luma, st_luma)):
    k = dict(c=c, n=n, st=st)
    assert run(v=None, **k) == E_ARG and run(i=None, **k) == E_ARG and run(o=None, **k) == E_ARG
    assert run(i=base + 1, **k) == E_ARG                                                 # an odd input base
    assert run(c=c, n=n, st=st + 1) == E_ARG and run(c=c, n=n, st=9 * n - 2) == E_ARG and run(c=c, n=n, st=0) == E_ARG      # an odd, a short stride
    assert run(o=obase + 4, **k) == E_ARG and run(o=obase + 8, **k) == E_ARG and run(o=obase + 2, **k) == E_ARG    # the output base: 16 bytes
    assert run(ost=ostride - 16, **k) == E_ARG and run(ost=ostride + 8, **k) == E_ARG and run(ost=ostride + 4, **k) == E_ARG and run(ost=0, **k) == E_ARG
    assert run(fmt=0, **k) == E_ARG and run(fmt=3, **k) == E_ARG and run(fw=0, **k) == E_ARG and run(x0=8, **k) == E_ARG and run(nf=65536, **k) == E_ARG
    # arguments before the truncated stream
    t = dict(c=c, n=n - 1, st=st)
    assert run(i=base + 1, **t) == E_ARG and run(o=obase + 4, **t) == E_ARG and run(v=None, **t) == E_ARG and run(ost=ostride + 8, **t) == E_ARG and run(x0=8, **t) == E_ARG
    assert run(c=c, n=n - 1, st=9 * (n - 1) - 1) == E_ARG
    # the truncated stream before the device
    assert run(**t) == E_HEADER and run(fmt=2, ost=144, **t) == E_HEADER
    # and only then the device
    assert run(**k) == NODEV and run(i=base + 2, **k) == NODEV and run(c=c, n=n, st=st + 2) == NODEV and run(ost=ostride + 16, **k) == NODEV and run(fmt=2, ost=144, **k) == NODEV
assert run(c=None) == E_ARG and run(c=compat) == E_ARG and run(c=raw) == E_ARG
# an empty batch, an empty window: T3_OK, no device asked for, null pointers allowed
assert run(nf=0) == OK and run(w=0, o=None, i=None, n=0) == OK and run(h=0) == OK
assert L.t3hip_decode_erasures_frames_window_async(None, C.c_uint64(0), C.c_uint64(0), C.c_uint32(0), None, C.c_uint64(0), C.c_uint32(0), C.c_uint32(0), C.c_uint32(0), C.c_uint32(0),
                                                   C.c_uint32(0), C.c_uint32(0), None, C.c_uint64(0), C.c_int(1), None, None) == OK
# one frame: the single-frame entry, the strides are not looked at, the output rule is its 4-byte rule
assert run(nf=1) == NODEV and run(nf=1, st=1, ost=1) == NODEV and run(nf=1, o=obase + 4) == NODEV and run(nf=1, o=obase + 2) == E_ARG and run(nf=1, i=base + 1) == E_ARG
assert run(nf=1, n=n_in - 1, st=1) == E_HEADER
seen = t3.DecoderContext(mode=1).cfg_last_seen
def dev(i=base, n=n_in, st=stride, nf=N, s=seen, fw=16, x0=2, w=9, o=obase, ost=ostride, fmt=1, c=cnt, r=rcs):
    return L.t3hip_decode_erasures_frames_window_dev(C.c_void_p(i), C.c_uint64(n), C.c_uint64(st), C.c_uint32(nf), C.byref(s) if s is not None else None, C.c_uint32(fw),
                                                     C.c_uint32(8), C.c_uint32(x0), C.c_uint32(1), C.c_uint32(w), C.c_uint32(5), C.c_void_p(o), C.c_uint64(ost), C.c_int(fmt), c, r, None)
def host(i=base, n=n_in, st=stride, nf=N, s=seen, fw=16, x0=2, w=9, o=obase, ost=ostride, fmt=1, c=cnt, r=rcs):
    return L.t3hip_decode_erasures_frames_window(C.c_void_p(i), C.c_uint64(n), C.c_uint64(st), C.c_uint32(nf), C.byref(s) if s is not None else None, C.c_uint32(fw),
                                                 C.c_uint32(8), C.c_uint32(x0), C.c_uint32(1), C.c_uint32(w), C.c_uint32(5), C.c_void_p(o), C.c_uint64(ost), C.c_int(fmt), c, r)
for fn in (dev, host):
    for n, st in ((n_in, stride), (n_luma, st_luma)):                                    # (the header tells the configuration: the word counts of both)
        k = dict(n=n, st=st)
        assert fn(s=None, **k) == E_ARG and fn(c=None, **k) == E_ARG and fn(r=None, **k) == E_ARG and fn(i=None, **k) == E_ARG and fn(o=None, **k) == E_ARG, fn.__name__
        assert fn(fmt=0, **k) == E_ARG and fn(fmt=3, **k) == E_ARG and fn(fw=0, **k) == E_ARG and fn(x0=8, **k) == E_ARG and fn(nf=65536, **k) == E_ARG, fn.__name__
        assert fn(s=compat, **k) == E_ARG and fn(s=raw, **k) == E_ARG and fn(n=n, st=9 * n - 2) == E_ARG and fn(ost=256, **k) == E_ARG, fn.__name__
        assert fn(**k) == NODEV and fn(fmt=2, ost=144, **k) == NODEV and fn(n=n, nf=1, st=1, ost=1) == NODEV, fn.__name__
    assert fn(n=9, i=None) == E_ARG and fn(n=9, s=compat) == E_ARG and fn(n=9, x0=8) == E_ARG      # arguments before the stream too short for a header
    assert fn(n=9) == E_HEADER and fn(n=9, fmt=2, ost=144) == E_HEADER and fn(n=9, nf=1) == E_HEADER, fn.__name__
    assert fn(nf=0) == OK and fn(nf=0, i=None, s=None, o=None, c=None, r=None) == OK, fn.__name__
    assert fn(w=0, o=None) == NODEV, fn.__name__                                         # an empty window still parses the headers: it needs the device
assert dev(i=base + 1) == E_ARG and dev(st=stride + 1) == E_ARG and dev(o=obase + 4) == E_ARG and dev(o=obase + 8) == E_ARG and dev(ost=ostride + 8) == E_ARG
assert dev(nf=1, o=obase + 4) == NODEV and dev(nf=1, o=obase + 2) == E_ARG
assert all(x == 0 for x in ver) and all(x == 0 for x in cnt) and all(x == 0 for x in rcs) and all(x == 0 for x in out) and all(x == 0 for x in buf)
print("ok")
"""


def test_arguments_then_the_device(built):
    """A process that never initialised a device: every bad argument is refused before the three batch entries ask for one, a truncated
    stream next, and only then T3_E_NODEVICE (no CPU fallback), on a path-1 and on a path-0 configuration; an empty batch is T3_OK with
    every pointer null; one frame is not refused for its strides.  Nothing is written anywhere.  (The addresses are host memory and never
    read: no device, no launch.)"""
    r = subprocess.run([sys.executable, "-c", NODEV % ROOT], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_batch_kernel_register_budget(built):
    """decode_era_frames_window_px<R, RGB, BCN> for the four codes, pixels and RGB, with and without beacon: built once each, no spilled
    VGPR, no scratch access inside the tile loop, 128 VGPRs at most (two 8-wave workgroups per CU) -- the budget of decode_era_window_px."""
    sys.path.insert(0, os.path.join(ROOT, "profiles"))
    import kernel_resources as kr
    ks = kr.all_kernels()
    loops = kr.loop_scratch(["t3_decode_era_frames_window.o"])
    hits = [n for n in ks if "decode_era_frames_window_px<" in n]
    assert len(hits) == 16, hits
    for n in hits:
        assert int(ks[n]["vgpr_spill_count"]) == 0 and int(ks[n]["vgpr_count"]) <= 128, (n, ks[n])
        assert loops[n] == (0, 0), (n, loops[n])


@pytest.mark.parametrize("which", range(4))
def test_masking_conditions(built, orc, which):
    """Every (stream, window) pair the GPU tests compare "outside refused tiles", from the yardstick alone: the mask leaves out at most
    half of that window's bytes, and every batch holds a frame compared in full -- so such a comparison cannot pass on a window that is
    mostly masked.  The GPU tests assert the same at run time."""
    import test_gpu_decode_erasures_frames_window as gw
    batches = gw.MASKED[which](built, orc)
    assert batches
    masked = 0
    for tag, fr, fars, win in batches:
        keeps = gw.mask_conditions(fr, fars, win, tag)
        masked += sum(1 for k in keeps if k is not None and not k.all())
    assert which in (1,) or masked > 0, which                                # (the address windows may hold no masked pixel at all)
