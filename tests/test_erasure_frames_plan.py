"""Host-only part of the batched repair with erasures (include/t3hip.h, "repair with erasures of a batch of equal FIXED frames"): the
refusals of the three entries in a process that never initialised a device -- bad arguments, then a truncated stream, only then
T3_E_NODEVICE --, and the register budget of erasure_frames_kernel<R>, the one tests/test_erasure_semantics.py pins for
erasure_fixed_kernel<R>.  The plan is t3hip_repair_frames_plan, unchanged (tests/test_repair_frames_plan.py).  The GPU side is
tests/test_gpu_erasure_frames.py."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    return ge.load_package()


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
buf = (C.c_uint8 * (N * max(stride, st_luma) + 32))(); ver = (C.c_uint32 * (6 * N))(); cnt = (C.c_uint32 * (6 * N))(); rcs = (C.c_int * N)()
base = C.addressof(buf); base += base & 1
p = t3.repair_frames_plan(n_raw, N, cfg); q = t3.repair_frames_plan(n_raw, N, luma)
assert p.one_launch == 1 and p.path == 1 and p.stride_min == stride and q.one_launch == 0 and q.path == 0 and q.stride_min == st_luma
def run(io=base, n=n_in, st=stride, nf=N, c=cfg, flags=1, v=C.addressof(ver)):
    return L.t3hip_repair_erasures_frames_async(C.c_void_p(io), C.c_uint64(n), C.c_uint64(st), C.c_uint32(nf), C.byref(c) if c is not None else None,
                                                C.c_uint64(n_raw), C.c_uint32(flags), C.c_void_p(v), None)
E_ARG, E_HEADER = -3, -5
assert run(c=None) == E_ARG and run(v=None) == E_ARG and run(io=None) == E_ARG and run(io=base + 1) == E_ARG
assert run(st=stride + 1) == E_ARG and run(st=9 * n_in - 2) == E_ARG and run(st=0) == E_ARG and run(flags=2) == E_ARG
assert run(c=compat) == E_ARG and run(c=raw) == E_ARG and run(nf=65536) == E_ARG
assert run(n=n_in - 1) == E_HEADER and run(n=n_luma - 1, st=st_luma, c=luma) == E_HEADER      # one launch (path 1) and loop (path 0) alike
assert run(nf=0) == t3.OK and run(nf=0, io=None, v=None) == t3.OK
assert run() == t3.E_NODEVICE and run(flags=0) == t3.E_NODEVICE and run(io=base + 2) == t3.E_NODEVICE and run(st=stride + 2) == t3.E_NODEVICE
assert run(n=n_luma, st=st_luma, c=luma) == t3.E_NODEVICE and run(nf=1) == t3.E_NODEVICE and run(nf=1, st=1) == t3.E_NODEVICE and run(nf=1, io=base + 1) == E_ARG
assert run(nf=1, n=n_in - 1, st=1) == E_HEADER
seen = t3.DecoderContext(mode=1).cfg_last_seen
def dev(io=base, st=stride, nf=N, s=seen, flags=1, c=cnt, r=rcs):
    return L.t3hip_repair_erasures_frames_dev(C.c_void_p(io), C.c_uint64(n_in), C.c_uint64(st), C.c_uint32(nf), C.byref(s) if s is not None else None, C.c_uint32(flags), c, r, None)
def host(io=base, st=stride, nf=N, s=seen, flags=1, c=cnt, r=rcs):
    return L.t3hip_repair_erasures_frames(C.c_void_p(io), C.c_uint64(n_in), C.c_uint64(st), C.c_uint32(nf), C.byref(s) if s is not None else None, C.c_uint32(flags), c, r)
for fn in (dev, host):
    assert fn(c=None) == E_ARG and fn(r=None) == E_ARG and fn(s=None) == E_ARG and fn(s=compat) == E_ARG and fn(s=raw) == E_ARG and fn(flags=2) == E_ARG, fn.__name__
    assert fn(io=None) == E_ARG and fn(st=9 * n_in - 2) == E_ARG and fn(nf=65536) == E_ARG, fn.__name__
    assert fn(nf=0) == t3.OK and fn(nf=0, io=None, c=None, r=None) == t3.OK and fn() == t3.E_NODEVICE and fn(nf=1, st=1) == t3.E_NODEVICE, fn.__name__
assert dev(io=base + 1) == E_ARG and dev(st=stride + 1) == E_ARG
assert all(x == 0 for x in ver) and all(x == 0 for x in cnt)                                   # nothing was written anywhere
print("ok")
"""


def test_arguments_then_the_device(built):
    """A process that never initialised a device: every bad argument is refused before the three batch entries ask for one, a truncated
    stream next (on a path-1 and on a path-0 configuration), and only then T3_E_NODEVICE (no CPU fallback); an empty batch is T3_OK, with
    null pointers too; one frame is not refused for its stride.  (The addresses are host memory and never read: no device, no launch.)"""
    r = subprocess.run([sys.executable, "-c", NODEV % ROOT], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_wrappers_exist(built):
    t3 = built
    for name in ("repair_erasures_frames_async", "repair_erasures_frames_dev", "repair_erasures_frames"):
        assert callable(getattr(t3, name)), name
    assert t3.repair_erasures_frames(__import__("numpy").zeros((0, 18), "uint8"), t3.DecoderContext(mode=1)) == (t3.OK, [], [])


def test_batch_kernel_register_budget(built):
    """erasure_frames_kernel<R> for the four codes: built once each, no spilled VGPR, no scratch access inside the tile loop, 128 VGPRs at
    most (two 8-wave workgroups per CU) -- the budget of erasure_fixed_kernel<R>; the batch header compare exists exactly once, the one of t3_repair_frames.hip with the
    verdict stride as an argument, and no second one for six words."""
    sys.path.insert(0, os.path.join(ROOT, "profiles"))
    import kernel_resources as kr
    ks = kr.all_kernels()
    loops = kr.loop_scratch(["t3_repair_era_frames.o"])
    assert len(loops) == 4, loops
    for r in (2, 4, 6, 8):
        hit = [n for n in ks if "erasure_frames_kernel<%d>" % r in n]
        assert len(hit) == 1, (r, hit)
        assert int(ks[hit[0]]["vgpr_spill_count"]) == 0 and int(ks[hit[0]]["vgpr_count"]) <= 128, (hit[0], ks[hit[0]])
        assert loops[hit[0]] == (0, 0), (hit[0], loops[hit[0]])
    assert len([n for n in ks if "hdr_compare_frames_kernel" in n]) == 1 and not [n for n in ks if "era_hdr_frames_kernel" in n]
