"""Host-only part of the batched stream repair (include/t3hip.h, "repair of a batch of equal FIXED frames"): the plan against the
single-frame plan, the refusals in a process that never initialised a device -- bad arguments, then a truncated stream, only then
T3_E_NODEVICE --, and the register budget of repair_frames_kernel<R>, the one tests/test_repair_semantics.py pins for
repair_fixed_kernel<R>.  The GPU side is tests/test_gpu_repair_frames.py."""
import os
import subprocess
import sys

import pytest

import rs_patterns as rp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = -3


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    return ge.load_package()


def _refused(t3, *a):
    with pytest.raises(t3.T3Error) as e:
        t3.repair_frames_plan(*a)
    return e.value.code


def test_frames_plan_over_configs(built):
    t3 = built
    for name, kw in rp.CONFIGS.items():
        cfg = t3.make_cfg(mode=1, **kw)
        for n_raw in (151, 40000):
            one = t3.repair_plan(n_raw, cfg); L = t3.plan(n_raw, cfg)
            for n_frames in (1, 2, 7):
                p = t3.repair_frames_plan(n_raw, n_frames, cfg)
                tag = (name, n_raw, n_frames)
                assert (p.n_frames, p.path, p.tiles_per_frame) == (n_frames, one.path, one.n_tiles), tag
                assert p.one_launch == (1 if one.path == 1 and n_frames >= 2 else 0), tag
                assert p.in_bytes == 9 * int(L.out_words) == one.in_bytes and p.stride_min == p.in_bytes + (p.in_bytes & 1), tag
        for bad in (t3.make_cfg(mode=0, **kw), t3.make_cfg(mode=1, **dict(kw, profile=0xFF))):      # COMPAT, RAW mode
            assert _refused(t3, 40000, 2, bad) == E_ARG, name
    assert _refused(t3, 100, 2, t3.make_cfg(mode=1, profile=2, uep=2, beacon=(4, 9, 1))) == E_ARG   # a FIXED limit: beacon slot >= 9
    assert t3.repair_frames_plan(40000, 0, t3.make_cfg(mode=1, **rp.CONFIGS["k20"])).one_launch == 0


def test_frames_plan_limits(built):
    t3 = built
    k20, luma = t3.make_cfg(mode=1, **rp.CONFIGS["k20"]), t3.make_cfg(mode=1, **rp.CONFIGS["luma"])
    assert t3.repair_frames_plan(40000, 65535, k20).one_launch == 1
    assert _refused(t3, 40000, 65536, k20) == E_ARG and _refused(t3, 40000, 65536, luma) == E_ARG
    # the one launch's tile space is 32-bit: n_frames * tiles_per_frame < 2^31 (host arithmetic, nothing is allocated)
    n_raw = 40_000_000
    one = t3.repair_plan(n_raw, k20)
    assert one.path == 1 and 65535 * one.n_tiles >= 1 << 31 > 2 * one.n_tiles
    ok = ((1 << 31) - 1) // one.n_tiles
    assert t3.repair_frames_plan(n_raw, ok, k20).one_launch == 1
    assert _refused(t3, n_raw, ok + 1, k20) == E_ARG and _refused(t3, n_raw, 65535, k20) == E_ARG
    p = t3.repair_frames_plan(n_raw, 65535, luma)                          # a loop of the single-frame body has no such limit
    assert p.one_launch == 0 and p.path == 0


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
stride = 9 * n_in + (9 * n_in & 1); st_luma = 9 * n_luma + (9 * n_luma & 1)
buf = (C.c_uint8 * (N * max(stride, st_luma) + 32))(); ver = (C.c_uint32 * (4 * N))(); cnt = (C.c_uint32 * (4 * N))(); rcs = (C.c_int * N)()
base = C.addressof(buf); base += base & 1
def run(io=base, n=n_in, st=stride, nf=N, c=cfg, flags=1, v=C.addressof(ver)):
    return L.t3hip_repair_frames_async(C.c_void_p(io), C.c_uint64(n), C.c_uint64(st), C.c_uint32(nf), C.byref(c) if c is not None else None, C.c_uint64(n_raw),
                                       C.c_uint32(flags), C.c_void_p(v), None)
E_ARG, E_HEADER = -3, -5
assert run(c=None) == E_ARG and run(v=None) == E_ARG and run(io=None) == E_ARG and run(io=base + 1) == E_ARG
assert run(st=stride + 1) == E_ARG and run(st=9 * n_in - 2) == E_ARG and run(st=0) == E_ARG and run(flags=2) == E_ARG
assert run(c=compat) == E_ARG and run(c=raw) == E_ARG and run(nf=65536) == E_ARG
assert run(n=n_in - 1) == E_HEADER and run(n=n_luma - 1, st=st_luma, c=luma) == E_HEADER      # one launch and loop alike
assert run(nf=0) == t3.OK and run(nf=0, io=None, v=None) == t3.OK
assert run() == t3.E_NODEVICE and run(flags=0) == t3.E_NODEVICE and run(io=base + 2) == t3.E_NODEVICE and run(st=stride + 2) == t3.E_NODEVICE
assert run(n=n_luma, st=st_luma, c=luma) == t3.E_NODEVICE and run(nf=1) == t3.E_NODEVICE and run(nf=1, st=1) == t3.E_NODEVICE and run(nf=1, io=base + 1) == E_ARG
seen = t3.DecoderContext(mode=1).cfg_last_seen
def dev(io=base, st=stride, nf=N, s=seen, flags=1, c=cnt, r=rcs):
    return L.t3hip_repair_frames_dev(C.c_void_p(io), C.c_uint64(n_in), C.c_uint64(st), C.c_uint32(nf), C.byref(s) if s is not None else None, C.c_uint32(flags), c, r, None)
def host(io=base, st=stride, nf=N, s=seen, flags=1, c=cnt, r=rcs):
    return L.t3hip_repair_frames(C.c_void_p(io), C.c_uint64(n_in), C.c_uint64(st), C.c_uint32(nf), C.byref(s) if s is not None else None, C.c_uint32(flags), c, r)
for fn in (dev, host):
    assert fn(c=None) == E_ARG and fn(r=None) == E_ARG and fn(s=None) == E_ARG and fn(s=compat) == E_ARG and fn(flags=2) == E_ARG, fn.__name__
    assert fn(io=None) == E_ARG and fn(st=9 * n_in - 2) == E_ARG and fn(nf=65536) == E_ARG, fn.__name__
    assert fn(nf=0) == t3.OK and fn() == t3.E_NODEVICE, fn.__name__
assert dev(io=base + 1) == E_ARG and dev(st=stride + 1) == E_ARG
p = t3.repair_frames_plan(n_raw, N, cfg)
assert p.one_launch == 1 and p.path == 1 and p.stride_min == stride
print("ok")
"""


def test_arguments_then_the_device(built):
    """A process that never initialised a device: every bad argument is refused before the batch entries ask for one, a truncated stream
    next, and only then T3_E_NODEVICE (no CPU fallback); an empty batch is T3_OK; the plan answers.  (The addresses are host memory and
    never read: no device, no launch.)"""
    r = subprocess.run([sys.executable, "-c", NODEV % ROOT], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_batch_kernel_register_budget(built):
    """repair_frames_kernel<R> for the four codes: built once each, no spilled VGPR, no scratch access inside the tile loop, 80 VGPRs at
    most (three 8-wave workgroups per CU) -- the budget of repair_fixed_kernel<R>; the batch header compare exists exactly once."""
    sys.path.insert(0, os.path.join(ROOT, "profiles"))
    import kernel_resources as kr
    ks = kr.all_kernels()
    loops = kr.loop_scratch(["t3_repair_frames.o"])
    for r in (2, 4, 6, 8):
        hit = [n for n in ks if "repair_frames_kernel<%d>" % r in n]
        assert len(hit) == 1, (r, hit)
        assert int(ks[hit[0]]["vgpr_spill_count"]) == 0 and int(ks[hit[0]]["vgpr_count"]) <= 80, (hit[0], ks[hit[0]])
        assert loops[hit[0]] == (0, 0), (hit[0], loops[hit[0]])
    assert len([n for n in ks if "hdr_compare_frames_kernel" in n]) == 1
