"""Host-only part of the decode with erasures (include/t3hip.h, "decode with erasures"): t3hip_decode_erasures_plan over every
configuration of tests/rs_patterns.py and every output format, the refusals of the three entries in a process that never initialised a
device -- bad arguments and T3_E_CAPACITY, then a truncated stream, only then T3_E_NODEVICE --, the exported symbols, and the register
budget of decode_era_px_kernel<R, RGB, BCN>.  The GPU side is tests/test_gpu_decode_erasures.py."""
import ctypes as C
import os
import subprocess
import sys

import pytest

import rs_patterns as rp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUSED = rp.ONE_K + ("k22_beacon2_slot8", "k20_beacon83")          # where the fused pixel decoder serves a frame
SYMBOLS = ("t3hip_decode_erasures_plan", "t3hip_decode_erasures_frame_async", "t3hip_decode_erasures_profile_dev", "t3hip_decode_erasures_profile")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    return ge.load_package()


def test_symbols_exported(built):
    """The four entries are in the built library and the mirror has their wrappers."""
    L = built.lib()
    for name in SYMBOLS:
        assert hasattr(L, name), name
    for name in ("decode_erasures_plan", "decode_erasures_frame_async", "decode_erasures_profile_dev", "decode_erasures_profile", "DecodeErasuresPlan"):
        assert callable(getattr(built, name)), name
    assert C.sizeof(built.DecodeErasuresPlan) == 32


@pytest.mark.parametrize("n_px", (301, 2 * 108 * 24 * 3 + 7, 1_000_001))
@pytest.mark.parametrize("name", sorted(rp.CONFIGS))
def test_path_per_configuration(built, name, n_px):
    """Path 1 exactly for one k, 1-D (beacon or not) with pixel or RGB output; everything else path 0.  n_tiles is the tile count of the
    window and repair planners for the frame (52 blocks of every band per tile); scratch_bytes is the private copy of path 0."""
    t3 = built
    cfg = t3.make_cfg(mode=1, **rp.CONFIGS[name])
    n_raw = (n_px + 1) // 2
    L = t3.plan(n_raw, cfg)
    tiles = -(-max(int(L.band_blocks[b]) for b in range(9)) // 52)
    for fmt in (0, 1, 2):
        p = t3.decode_erasures_plan(n_raw, cfg, fmt)
        want = 1 if (name in FUSED and fmt in (1, 2)) else 0
        assert p.path == want, (name, fmt, p.path)
        assert p.in_bytes == 9 * int(L.out_words) and p.out_units == (n_raw if fmt == 0 else 2 * n_raw), (name, fmt)
        if want:
            assert p.n_tiles == tiles and p.scratch_bytes == 0, (name, fmt, p.n_tiles, tiles)
            if name in rp.ONE_K:
                assert p.n_tiles == t3.repair_plan(n_raw, cfg).n_tiles == t3.window_plan(n_raw, cfg, 2 * n_raw, 1, 0, 0, 2 * n_raw, 1).n_tiles, (name, fmt)
        else:
            assert p.n_tiles == 0 and p.scratch_bytes == (p.in_bytes + 15) // 16 * 16, (name, fmt)


def test_plan_refusals(built):
    t3 = built; L = t3.lib()
    cfg = t3.make_cfg(profile=2, uep=2, mode=1)
    p = t3.DecodeErasuresPlan()
    plan = lambda c, fmt, out=p: L.t3hip_decode_erasures_plan(C.c_uint64(64), C.byref(c) if c is not None else None, C.c_int(fmt), C.byref(out) if out is not None else None)
    assert plan(cfg, 1) == t3.OK and plan(None, 1) == t3.E_ARG and plan(cfg, 1, None) == t3.E_ARG and plan(cfg, 3) == t3.E_ARG and plan(cfg, -1) == t3.E_ARG
    assert plan(t3.make_cfg(profile=2, uep=2, mode=0), 1) == t3.E_ARG                   # COMPAT
    assert plan(t3.make_cfg(profile=0xFF, mode=1), 1) == t3.E_ARG                       # RAW mode
    assert t3.decode_erasures_plan(0, cfg, 1).path == 0                                 # an empty frame: nothing for the fused kernel


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
buf = (C.c_uint8 * (9 * max(n_in, n_luma) + 64))(); out = (C.c_uint8 * (18 * n_raw + 64))(); ver = (C.c_uint32 * 4)(); cnt = (C.c_uint32 * 4)()
base = C.addressof(buf); base += -base %% 16
obase = C.addressof(out); obase += -obase %% 16
n_out = C.c_uint64()
def run(i=base, n=n_in, c=cfg, o=obase, cap=2 * n_raw, no=n_out, fmt=1, v=C.addressof(ver)):
    return L.t3hip_decode_erasures_frame_async(C.c_void_p(i), C.c_uint64(n), C.byref(c) if c is not None else None, C.c_uint64(n_raw), C.c_void_p(o), C.c_uint64(cap),
                                               C.byref(no) if no is not None else None, C.c_int(fmt), C.c_void_p(v), None)
E_ARG, E_HEADER, E_CAP = t3.E_ARG, t3.E_HEADER, t3.E_CAPACITY
assert run(c=None) == E_ARG and run(v=None) == E_ARG and run(no=None) == E_ARG and run(i=None) == E_ARG and run(i=base + 1) == E_ARG and run(o=None) == E_ARG
assert run(fmt=3) == E_ARG and run(c=compat) == E_ARG and run(c=raw) == E_ARG
assert run(o=obase + 1) == E_ARG and run(o=obase + 2) == E_ARG                      # path 1: one launch or refused, never silently path 0
assert run(cap=2 * n_raw - 1) == E_CAP and n_out.value == 2 * n_raw and run(cap=n_raw - 1, fmt=0) == E_CAP and n_out.value == n_raw
assert run(cap=2 * n_raw - 1, n=n_in - 1) == E_CAP                                  # capacity before the truncated stream
assert run(n=n_in - 1) == E_HEADER and run(n=n_in - 1, fmt=0) == E_HEADER and run(n=n_luma - 1, c=luma) == E_HEADER    # path 1 and path 0 alike
assert run(n=n_in - 1, i=base + 1) == E_ARG                                         # arguments before the truncated stream
assert run() == t3.E_NODEVICE and run(i=base + 2) == t3.E_NODEVICE and run(fmt=2) == t3.E_NODEVICE and run(fmt=0, cap=n_raw) == t3.E_NODEVICE
assert run(fmt=0, cap=n_raw, o=obase + 1) == t3.E_NODEVICE and run(n=n_luma, c=luma, o=obase + 2) == t3.E_NODEVICE      # path 0: the plain decoders' addresses
seen = t3.DecoderContext(mode=1).cfg_last_seen
def dev(i=base, s=seen, o=obase, no=n_out, fmt=1, c=cnt):
    return L.t3hip_decode_erasures_profile_dev(C.c_void_p(i), C.c_uint64(n_in), C.byref(s) if s is not None else None, C.c_void_p(o), C.c_uint64(2 * n_raw),
                                               C.byref(no) if no is not None else None, C.c_int(fmt), c, None)
def host(i=base, s=seen, o=obase, no=n_out, fmt=1, c=cnt):
    return L.t3hip_decode_erasures_profile(C.c_void_p(i), C.c_uint64(n_in), C.byref(s) if s is not None else None, C.c_void_p(o), C.c_uint64(2 * n_raw),
                                           C.byref(no) if no is not None else None, C.c_int(fmt), c)
for fn in (dev, host):
    assert fn(s=None) == E_ARG and fn(c=None) == E_ARG and fn(no=None) == E_ARG and fn(i=None) == E_ARG and fn(fmt=3) == E_ARG, fn.__name__
    assert fn(s=compat) == E_ARG and fn(s=raw) == E_ARG and fn() == t3.E_NODEVICE, fn.__name__
assert dev(i=base + 1) == E_ARG
assert all(x == 0 for x in ver) and all(x == 0 for x in cnt) and all(x == 0 for x in out)      # nothing was written anywhere
print("ok")
"""


def test_arguments_then_the_device(built):
    """A process that never initialised a device: bad arguments and a short output are refused before the entries ask for one, a truncated
    stream next (on a path-1 and on a path-0 configuration), and only then T3_E_NODEVICE (no CPU fallback).  (The addresses are host
    memory and never read: no device, no launch.)"""
    r = subprocess.run([sys.executable, "-c", NODEV % ROOT], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_kernel_register_budget(built):
    """decode_era_px_kernel<R, RGB, BCN> for the four codes, pixels and RGB, with and without beacon: built once each, no spilled VGPR, no
    scratch access inside the tile loop, 128 VGPRs at most (two 8-wave workgroups per CU)."""
    sys.path.insert(0, os.path.join(ROOT, "profiles"))
    import kernel_resources as kr
    ks = kr.all_kernels()
    loops = kr.loop_scratch(["t3_decode_era.o"])
    hits = [n for n in ks if "decode_era_px_kernel<" in n]
    assert len(hits) == 16, hits
    for n in hits:
        assert int(ks[n]["vgpr_spill_count"]) == 0 and int(ks[n]["vgpr_count"]) <= 128, (n, ks[n])
        assert loops[n] == (0, 0), (n, loops[n])
