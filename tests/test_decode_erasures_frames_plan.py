"""Host-only part of the batched decode with erasures (include/t3hip.h, "decode with erasures of a batch of equal FIXED frames"):
t3hip_decode_erasures_frames_plan over every configuration of tests/rs_patterns.py, every output format and three batch sizes, the
refusals of the three entries in a process that never initialised a device -- bad arguments, then a truncated stream, only then
T3_E_NODEVICE --, the exported symbols, and the register budget of decode_era_frames_px<R, RGB, BCN>.  The GPU side is
tests/test_gpu_decode_erasures_frames.py."""
import ctypes as C
import os
import subprocess
import sys

import pytest

import rs_patterns as rp
from test_decode_erasures_plan import FUSED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("t3hip_decode_erasures_frames_plan", "t3hip_decode_erasures_frames_async", "t3hip_decode_erasures_frames_dev", "t3hip_decode_erasures_frames")
UNIT = {0: 9, 1: 6, 2: 3}


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    return ge.load_package()


def test_symbols_exported(built):
    """The four entries are in the built library, the mirror has their wrappers, and the ctypes struct has the C struct's size: the
    single-frame plan (32 bytes), n_frames, one_launch and padding (8), four 64-bit fields."""
    L = built.lib()
    for name in SYMBOLS:
        assert hasattr(L, name), name
    for name in ("DecodeErasuresFramesPlan", "decode_erasures_frames_plan", "decode_erasures_frames_async", "decode_erasures_frames_dev", "decode_erasures_frames"):
        assert callable(getattr(built, name)), name
    assert C.sizeof(built.DecodeErasuresFramesPlan) == C.sizeof(built.DecodeErasuresPlan) + 8 + 4 * 8 == 72
    # the C side writes exactly that many bytes: the struct sits in front of a guard that must survive
    class Guarded(C.Structure):
        _fields_ = [("p", built.DecodeErasuresFramesPlan), ("guard", C.c_uint8 * 64)]
    g = Guarded(); C.memset(C.byref(g), 0xA5, C.sizeof(g))
    cfg = built.make_cfg(mode=1, **rp.CONFIGS["k20"])
    assert L.t3hip_decode_erasures_frames_plan(C.c_uint64(151), C.c_uint32(5), C.byref(cfg), C.c_int(1), C.byref(g.p)) == built.OK
    assert bytes(g.guard) == b"\xA5" * 64 and g.p.n_frames == 5 and g.p.scratch_bytes == 0 and g.p.out_bytes == 6 * 302 and list(g.p.pad_) == [0, 0, 0]
    assert built.decode_erasures_frames(__import__("numpy").zeros((0, 18), "uint8"), built.DecoderContext(mode=1), 1) == (built.OK, [], [], [])


@pytest.mark.parametrize("n_px", (301, 1_000_001))
@pytest.mark.parametrize("name", sorted(rp.CONFIGS))
def test_plan_per_configuration(built, name, n_px):
    """one_launch exactly where the single-frame plan says path 1 and the batch has two frames at least; `frame` is
    t3hip_decode_erasures_plan's struct; the input stride minimum is the frame's bytes rounded up to even, the output's its bytes rounded
    up to 16; the one-launch path holds no scratch, the loop one frame's."""
    t3 = built
    cfg = t3.make_cfg(mode=1, **rp.CONFIGS[name])
    n_raw = (n_px + 1) // 2
    for fmt in (0, 1, 2):
        single = t3.decode_erasures_plan(n_raw, cfg, fmt)
        assert single.path == (1 if name in FUSED and fmt != 0 else 0)
        for n_frames in (1, 2, 5):
            p = t3.decode_erasures_frames_plan(n_raw, n_frames, cfg, fmt)
            tag = (name, n_px, fmt, n_frames)
            assert p.one_launch == (1 if single.path == 1 and n_frames >= 2 else 0), tag
            assert bytes(p.frame) == bytes(single) and p.n_frames == n_frames, tag
            assert p.in_stride_min == single.in_bytes + single.in_bytes % 2, tag
            assert p.out_bytes == single.out_units * UNIT[fmt] and p.out_stride_min == (p.out_bytes + 15) // 16 * 16, tag
            assert p.scratch_bytes == (0 if p.one_launch else single.scratch_bytes), tag
            if p.one_launch:
                assert p.scratch_bytes == 0 and p.frame.n_tiles > 0, tag


def test_plan_refusals(built):
    t3 = built; L = t3.lib()
    cfg = t3.make_cfg(profile=2, uep=2, mode=1)
    p = t3.DecodeErasuresFramesPlan()
    def plan(c, fmt, out=p, n=5, n_raw=64):
        return L.t3hip_decode_erasures_frames_plan(C.c_uint64(n_raw), C.c_uint32(n), C.byref(c) if c is not None else None, C.c_int(fmt), C.byref(out) if out is not None else None)
    assert plan(cfg, 1) == t3.OK and plan(None, 1) == t3.E_ARG and plan(cfg, 1, None) == t3.E_ARG and plan(cfg, 3) == t3.E_ARG and plan(cfg, -1) == t3.E_ARG
    assert plan(t3.make_cfg(profile=2, uep=2, mode=0), 1) == t3.E_ARG                   # COMPAT
    assert plan(t3.make_cfg(profile=0xFF, mode=1), 1) == t3.E_ARG                       # RAW mode
    assert plan(cfg, 1, n=65535) == t3.OK and plan(cfg, 1, n=65536) == t3.E_ARG and plan(cfg, 0, n=65536) == t3.E_ARG
    assert plan(cfg, 1, n=0) == t3.OK and p.one_launch == 0 and p.n_frames == 0
    # the one launch's tile space is 32-bit: a k20 pixel tile holds 2160 pixels
    n_raw = 32768 * 1080
    one = t3.decode_erasures_plan(n_raw, cfg, 1)
    assert one.path == 1 and one.n_tiles == 32768 and 65535 * one.n_tiles < 2 ** 31 <= 65535 * (one.n_tiles + 1)
    assert plan(cfg, 1, n=65535, n_raw=n_raw) == t3.OK and plan(cfg, 1, n=65535, n_raw=n_raw + 1080) == t3.E_ARG
    assert plan(cfg, 0, n=65535, n_raw=n_raw + 1080) == t3.OK and plan(cfg, 1, n=1, n_raw=n_raw + 1080) == t3.OK      # the loop has no such bound
    assert t3.decode_erasures_frames_plan(0, 5, cfg, 1).one_launch == 0                 # empty frames: nothing for the fused kernel


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
p = t3.decode_erasures_frames_plan(n_raw, N, cfg, 1); q = t3.decode_erasures_frames_plan(n_raw, N, luma, 1); w = t3.decode_erasures_frames_plan(n_raw, N, cfg, 0)
assert p.one_launch == 1 and q.one_launch == 0 and w.one_launch == 0 and p.frame.path == 1 and q.frame.path == 0
stride = p.in_stride_min; st_luma = q.in_stride_min; ostride = p.out_stride_min
assert stride == 9 * n_in + (9 * n_in & 1) and ostride == (12 * n_raw + 15) // 16 * 16 and w.out_stride_min == 9 * n_raw
buf = (C.c_uint8 * (N * max(stride, st_luma) + 64))(); out = (C.c_uint8 * (N * (ostride + 16) + 64))(); ver = (C.c_uint32 * (4 * N))(); cnt = (C.c_uint32 * (4 * N))()
rcs = (C.c_int * N)(); n_out = C.c_uint64()
base = C.addressof(buf); base += -base %% 16
obase = C.addressof(out); obase += -obase %% 16
E_ARG, E_HEADER, NODEV, OK = t3.E_ARG, t3.E_HEADER, t3.E_NODEVICE, t3.OK
def run(i=base, n=n_in, st=stride, nf=N, c=cfg, o=obase, ost=ostride, fmt=1, v=C.addressof(ver)):
    return L.t3hip_decode_erasures_frames_async(C.c_void_p(i), C.c_uint64(n), C.c_uint64(st), C.c_uint32(nf), C.byref(c) if c is not None else None, C.c_uint64(n_raw),
                                                C.c_void_p(o), C.c_uint64(ost), C.c_int(fmt), C.c_void_p(v), None)
# every class of bad argument
assert run(c=None) == E_ARG and run(v=None) == E_ARG and run(i=None) == E_ARG and run(o=None) == E_ARG
assert run(i=base + 1) == E_ARG and run(st=stride + 1) == E_ARG and run(st=9 * n_in - 2) == E_ARG and run(st=0) == E_ARG
assert run(o=obase + 8) == E_ARG and run(o=obase + 2) == E_ARG and run(ost=ostride + 8) == E_ARG and run(ost=ostride - 16) == E_ARG and run(ost=0) == E_ARG
assert run(fmt=0, o=obase + 8) == E_ARG and run(fmt=0, ost=w.out_stride_min + 8) == E_ARG      # the output rule holds on the loop path too
assert run(fmt=3) == E_ARG and run(fmt=-1) == E_ARG and run(c=compat) == E_ARG and run(c=raw) == E_ARG and run(nf=65536) == E_ARG
# arguments before the truncated stream; the truncated stream before the device, on a path-1 and on a path-0 configuration
assert run(n=n_in - 1, i=base + 1) == E_ARG and run(n=n_in - 1, o=obase + 8) == E_ARG and run(n=n_in - 1, v=None) == E_ARG and run(n=n_in - 1, st=9 * (n_in - 1) - 1) == E_ARG
assert run(n=n_in - 1) == E_HEADER and run(n=n_in - 1, fmt=0) == E_HEADER and run(n=n_luma - 1, st=st_luma, c=luma) == E_HEADER
assert run(nf=0) == OK and L.t3hip_decode_erasures_frames_async(None, C.c_uint64(0), C.c_uint64(0), C.c_uint32(0), None, C.c_uint64(0), None, C.c_uint64(0), C.c_int(1), None, None) == OK
assert run() == NODEV and run(i=base + 2) == NODEV and run(st=stride + 2) == NODEV and run(ost=ostride + 16) == NODEV and run(fmt=2) == NODEV
assert run(fmt=0, ost=w.out_stride_min) == NODEV and run(n=n_luma, st=st_luma, c=luma) == NODEV
# one frame: the single-frame entry, the strides are not looked at
assert run(nf=1) == NODEV and run(nf=1, st=1, ost=1) == NODEV and run(nf=1, i=base + 1) == E_ARG and run(nf=1, n=n_in - 1, st=1) == E_HEADER and run(nf=1, o=obase + 2) == E_ARG
seen = t3.DecoderContext(mode=1).cfg_last_seen
def dev(i=base, n=n_in, st=stride, nf=N, s=seen, o=obase, ost=ostride, cap=2 * n_raw, no=n_out, fmt=1, c=cnt, r=rcs):
    return L.t3hip_decode_erasures_frames_dev(C.c_void_p(i), C.c_uint64(n), C.c_uint64(st), C.c_uint32(nf), C.byref(s) if s is not None else None, C.c_void_p(o),
                                              C.c_uint64(ost), C.c_uint64(cap), C.byref(no) if no is not None else None, C.c_int(fmt), c, r, None)
def host(i=base, n=n_in, st=stride, nf=N, s=seen, o=obase, ost=ostride, cap=2 * n_raw, no=n_out, fmt=1, c=cnt, r=rcs):
    return L.t3hip_decode_erasures_frames(C.c_void_p(i), C.c_uint64(n), C.c_uint64(st), C.c_uint32(nf), C.byref(s) if s is not None else None, C.c_void_p(o),
                                          C.c_uint64(ost), C.c_uint64(cap), C.byref(no) if no is not None else None, C.c_int(fmt), c, r)
for fn in (dev, host):
    assert fn(s=None) == E_ARG and fn(no=None) == E_ARG and fn(c=None) == E_ARG and fn(r=None) == E_ARG and fn(i=None) == E_ARG and fn(o=None) == E_ARG, fn.__name__
    assert fn(fmt=3) == E_ARG and fn(s=compat) == E_ARG and fn(s=raw) == E_ARG and fn(nf=65536) == E_ARG, fn.__name__
    assert fn(st=9 * n_in - 2) == E_ARG and fn(ost=12 * n_raw - 16) == E_ARG, fn.__name__
    assert fn(n=9, st=stride, i=None) == E_ARG and fn(n=9, s=compat) == E_ARG       # arguments before the stream too short for a header
    assert fn(n=9) == E_HEADER and fn(n=9, fmt=0, cap=n_raw) == E_HEADER, fn.__name__
    assert fn(nf=0) == OK and fn(nf=0, i=None, s=None, o=None, no=None, c=None, r=None) == OK, fn.__name__
    assert fn() == NODEV and fn(fmt=0, cap=n_raw) == NODEV and fn(fmt=2) == NODEV and fn(nf=1, st=1, ost=1) == NODEV, fn.__name__
assert dev(i=base + 1) == E_ARG and dev(st=stride + 1) == E_ARG and dev(o=obase + 8) == E_ARG and dev(ost=ostride + 8) == E_ARG
assert all(x == 0 for x in ver) and all(x == 0 for x in cnt) and all(x == 0 for x in rcs) and all(x == 0 for x in out) and all(x == 0 for x in buf) and n_out.value == 0
print("ok")
"""


def test_arguments_then_the_device(built):
    """A process that never initialised a device: every bad argument is refused before the three batch entries ask for one, a truncated
    stream next (on a path-1 and on a path-0 configuration), and only then T3_E_NODEVICE (no CPU fallback); an empty batch is T3_OK with
    every pointer null; one frame is not refused for its strides.  Nothing is written anywhere.  (The addresses are host memory and never
    read: no device, no launch.)"""
    r = subprocess.run([sys.executable, "-c", NODEV % ROOT], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_batch_kernel_register_budget(built):
    """decode_era_frames_px<R, RGB, BCN> for the four codes, pixels and RGB, with and without beacon: built once each, no spilled VGPR, no
    scratch access inside the tile loop, 128 VGPRs at most (two 8-wave workgroups per CU) -- the budget of decode_era_px_kernel."""
    sys.path.insert(0, os.path.join(ROOT, "profiles"))
    import kernel_resources as kr
    ks = kr.all_kernels()
    loops = kr.loop_scratch(["t3_decode_era_frames.o"])
    hits = [n for n in ks if "decode_era_frames_px<" in n]
    assert len(hits) == 16, hits
    for n in hits:
        assert int(ks[n]["vgpr_spill_count"]) == 0 and int(ks[n]["vgpr_count"]) <= 128, (n, ks[n])
        assert loops[n] == (0, 0), (n, loops[n])
