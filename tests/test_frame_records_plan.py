"""CPU-side checks of the batched frame records (N equal frames in one pass, include/t3hip.h; no GPU): the plan -- which CRC kernel
a frame gets, the waves its rounds are strided over, workgroups and partials per frame, one pass or the loop -- the argument limits,
that the device entries check their arguments before they ask for a device, and the three new kernels as built."""
import os
import sys
import tempfile

import numpy as np
import pytest

from test_crc_isa import CSRC, code_object, kernel_text, symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_CU = 256
SLOT_MOST = 64 + 8 * 1024                          # what t3hip_frame_record_scratch_bytes asks for one frame: the most a slot uses


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    return ge.load_package()


def r16(x):
    return (x + 15) & ~15


def expect(n_words, n_cu, slot, atomics=False, tables=False):
    """plan_crc's arithmetic for one frame of n_words coded words on a part with n_cu CUs, the frame's slot being `slot` bytes:
    (form, W, workgroups per frame, partials per frame)."""
    n_bytes = 9 * n_words
    rounds, tail = n_bytes // 2048, n_bytes % 2048
    if rounds < 64 or tables:                      # the table kernel: 2304-byte chunks, 256 per workgroup, accumulators
        chunks = -(-n_bytes // 2304)
        return 0, 0, -(-chunks // 256), 0
    slots = 8 * n_cu
    w = lambda l: max(4, (slots >> l) & ~3)
    l = 0
    while l < 7 and 8 * w(l) > rounds:
        l += 1
    wgs = w(l) // 4 + (1 if tail else 0)
    return 1, w(l), wgs, (wgs if slot >= 64 + 8 * wgs and not atomics else 0)


def words_for(rounds, tail):
    """A word count n near `rounds` rounds with 9 n = 2048 m + tail (tests/test_crc_tail.py)."""
    base = 2048 * rounds // 9
    n = base + ((tail * pow(9, -1, 2048) - base) % 2048)
    assert (9 * n) % 2048 == tail
    return n


# every level of the 256-CU part from both sides of its edge (8 W rounds), rests none / shortest / longest, and the table kernel's range
PLAN_WORDS = [0, 5, 100, words_for(40, 7), words_for(63, 2047)] + \
             [words_for(r, t) for w in (16, 32, 64, 128, 256, 512, 1024, 2048) for r in (8 * w - 1, 8 * w) for t in (0, 1, 2047)] + \
             [words_for(64, 0), words_for(64, 2047), 256604, 20766726]


@pytest.mark.parametrize("n_frames", [2, 3, 16, 65535])
def test_plan_arithmetic(built, n_frames):
    t3 = built
    for n_words in PLAN_WORDS:
        full = t3.frame_records_scratch_bytes(n_words, n_frames)
        assert full == SLOT_MOST * n_frames == t3.frame_record_scratch_bytes(n_words) * n_frames
        for scratch in (full, 16 * n_frames, 16 * n_frames + 15, (64 + 8 * 33) * n_frames, (64 + 8 * 33) * n_frames - 1, 10 * full):
            slot = min((scratch // n_frames) & ~15, SLOT_MOST)
            p = t3.frame_records_plan(n_words, n_frames, N_CU, scratch)
            form, w, wgs, parts = expect(n_words, N_CU, slot)
            assert (p.n_frames, p.one_pass) == (n_frames, 1), (n_words, scratch)
            assert (p.form, p.stride_waves, p.wgs_per_frame, p.partials_per_frame) == (form, w, wgs, parts), (n_words, scratch)
            assert (p.frame_bytes, p.stride_min, p.scratch_bytes) == (9 * n_words, r16(9 * n_words), slot * n_frames), (n_words, scratch)
    # the batch workload the entry is for: a coded 854 x 480 frame gets 128 of the part's 2048 wave slots, 16 of them fill it
    video = t3.encoded_words(854 * 480 // 2, t3.make_cfg(profile=2, uep=2, mode=t3.MODE_FIXED))       # FIXED RS(26,20): 1,127 rounds and a rest
    assert 9 * video // 2048 == 1127 and 9 * video % 2048
    p = t3.frame_records_plan(video, 16, N_CU)
    assert (p.form, p.stride_waves, p.wgs_per_frame, p.partials_per_frame) == (t3.RECORDS_FP4, 128, 33, 33)
    # another part: the levels follow its CU count
    for n_cu in (1, 64, 304):
        for n_words in PLAN_WORDS:
            p = t3.frame_records_plan(n_words, 3, n_cu)
            assert (p.form, p.stride_waves, p.wgs_per_frame, p.partials_per_frame) == expect(n_words, n_cu, SLOT_MOST), (n_cu, n_words)


def test_plan_loop_cases_and_knobs(built, monkeypatch):
    """One frame, T3HIP_CRC_BLOCKED and streams of 2^40 bytes or more are the loop of the single-frame entry; the other two knobs keep
    the one pass and change what a frame gets."""
    t3 = built
    n = words_for(255, 3)
    assert t3.frame_records_plan(n, 1, N_CU).one_pass == 0
    assert t3.frame_records_plan(n, 0, N_CU, 0).n_frames == 0 and t3.frame_records_plan(n, 0, N_CU, 0).one_pass == 0
    assert t3.frame_records_plan((1 << 40) // 9 + 1, 2, N_CU).one_pass == 0
    assert t3.frame_records_plan((1 << 40) // 9 - 1, 2, N_CU).one_pass == 1
    with monkeypatch.context() as m:
        m.setenv("T3HIP_CRC_BLOCKED", "1")
        assert t3.frame_records_plan(n, 3, N_CU).one_pass == 0
    with monkeypatch.context() as m:
        m.setenv("T3HIP_CRC_ATOMICS", "1")
        p = t3.frame_records_plan(n, 3, N_CU)
        assert (p.one_pass, p.form, p.stride_waves, p.wgs_per_frame, p.partials_per_frame) == (1,) + expect(n, N_CU, SLOT_MOST, atomics=True)
        assert p.partials_per_frame == 0 and p.wgs_per_frame > 0
    with monkeypatch.context() as m:
        m.setenv("T3HIP_CRC_TABLES", "1")
        p = t3.frame_records_plan(n, 3, N_CU)
        assert (p.one_pass, p.form, p.stride_waves, p.wgs_per_frame, p.partials_per_frame) == (1,) + expect(n, N_CU, SLOT_MOST, tables=True)
        assert p.form == t3.RECORDS_TABLES
    assert t3.frame_records_plan(n, 3, N_CU).form == t3.RECORDS_FP4


def test_plan_limits(built):
    """More than 65535 frames, a null plan, a scratch below 16 bytes per frame, a word count whose bytes overflow: T3_E_ARG."""
    import ctypes as C
    t3 = built
    assert t3.frame_records_plan(100, 65535, N_CU).one_pass == 1
    for kw in (dict(n_frames=65536), dict(n_frames=3, scratch_bytes=47), dict(n_words=1 << 60, n_frames=2, scratch_bytes=1 << 20)):
        with pytest.raises(t3.T3Error) as e:
            t3.frame_records_plan(kw.get("n_words", 100), kw["n_frames"], N_CU, kw.get("scratch_bytes"))
        assert e.value.code == t3.E_ARG, kw
    assert t3.lib().t3hip_frame_records_plan(C.c_uint64(100), C.c_uint32(3), C.c_uint32(N_CU), C.c_uint64(1 << 20), None) == t3.E_ARG


def test_entries_check_arguments_then_the_device(built):
    """The device entries refuse what is wrong with their arguments before they ask for a device -- a null or misaligned base, a stride
    that is no multiple of 16 or below the minimum, a misaligned or too small scratch, null records, no configuration, too many frames:
    T3_E_ARG -- and only then T3_E_NODEVICE (no CPU fallback); the plan for "the current device" needs one too.  (The addresses are
    never read: no device, no launch.)"""
    t3 = built
    if t3.is_ready():
        pytest.skip("a context exists in this process")
    cfg = t3.make_cfg(profile=2, uep=2, mode=t3.MODE_FIXED)
    n_words, n = 4861, 3
    smin = r16(9 * n_words)
    A, R, S = 1 << 20, 1 << 24, 1 << 25                       # three aligned addresses
    full = t3.frame_records_scratch_bytes(n_words, n)

    def rec(d=A, stride=smin, nf=n, cfg=cfg, recs=R, scr=S, scr_bytes=full, words=n_words):
        t3.frame_records_dev(d, words, stride, nf, 0, 1, cfg, recs, scr, scr_bytes)

    bad = [dict(d=0), dict(d=A + 8), dict(stride=smin + 8), dict(stride=smin - 16), dict(scr=S + 8), dict(scr=0), dict(scr_bytes=16 * n - 1),
           dict(recs=0), dict(cfg=None), dict(nf=65536, scr_bytes=1 << 30), dict(d=0, nf=1), dict(scr=S + 8, nf=1), dict(words=1 << 60)]
    for kw in bad:
        with pytest.raises(t3.T3Error) as e:
            rec(**kw)
        assert e.value.code == t3.E_ARG, kw
    for kw in (dict(), dict(nf=0), dict(nf=1), dict(scr_bytes=16 * n), dict(stride=smin + 4112), dict(d=0, words=0, stride=0)):
        with pytest.raises(t3.T3Error) as e:
            rec(**kw)
        assert e.value.code == t3.E_NODEVICE, kw
    crc = lambda d=A, n_bytes=9 * n_words, stride=smin, nf=n: t3.crc32_frames_dev(d, n_bytes, stride, nf)
    for kw in (dict(d=0), dict(d=A + 4), dict(stride=smin + 4), dict(stride=smin - 16), dict(nf=65536)):
        with pytest.raises(t3.T3Error) as e:
            crc(**kw)
        assert e.value.code == t3.E_ARG, kw
    for kw in (dict(), dict(nf=0), dict(nf=1), dict(d=0, n_bytes=0, stride=0)):
        with pytest.raises(t3.T3Error) as e:
            crc(**kw)
        assert e.value.code == t3.E_NODEVICE, kw
    with pytest.raises(t3.T3Error) as e:
        t3.crc32_frames([np.zeros(90, np.uint8)] * 2)
    assert e.value.code == t3.E_NODEVICE
    with pytest.raises(ValueError):
        t3.crc32_frames([np.zeros(90, np.uint8), np.zeros(99, np.uint8)])
    with pytest.raises(t3.T3Error) as e:
        t3.frame_records_plan(n_words, n, 0)                  # n_cu = 0: the current context's device
    assert e.value.code == t3.E_NODEVICE


NEW_KERNELS = ["crc_fp4_frames_kernel(", "crc_chunks_frames_kernel(", "frame_records_kernel("]


def test_new_kernels_register_budget(built):
    """The three batch kernels are built, once each, spill no VGPR and use no scratch (as their single-stream twins, which
    test_no_vgpr_spills_in_hot_kernels and the parent's resource lines hold to the same)."""
    sys.path.insert(0, os.path.join(ROOT, "profiles"))
    import kernel_resources as kr
    ks = kr.all_kernels()
    for want in NEW_KERNELS:
        hit = [n for n in ks if want in n]
        assert len(hit) == 1, (want, hit)
        k = ks[hit[0]]
        assert int(k["vgpr_spill_count"]) == 0 and int(k["sgpr_spill_count"]) == 0 and int(k["private_segment_fixed_size"]) == 0, (hit[0], k)
    bodies = kr.kernel_bodies(kr.CSRC, ["t3_crc_frames.o"])
    assert sorted(bodies) == sorted(n for n in ks if any(w in n for w in NEW_KERNELS)), "the new unit holds exactly the three kernels"
    for name, (_, body, _) in bodies.items():
        assert not [t for _, t, _ in body if t.startswith("scratch_")], name


@pytest.fixture(scope="module")
def frames_co(built):
    with tempfile.TemporaryDirectory() as td:
        co = code_object(os.path.join(CSRC, "t3_crc_frames.o"), td)
        yield co


def test_fp4_frames_kernel_prologue(frames_co):
    """crc_fp4_frames_kernel keeps crc_fp4_kernel's entry (tests/test_crc_prologue_isa.py): no barrier in front of the round loop, and
    no vector load of any kind in front of the first payload load."""
    import re
    body = kernel_text(frames_co, "_ZN2t321crc_fp4_frames_kernel")
    first = lambda prefix: [i for i, s in enumerate(body) if s.startswith(prefix)][0]
    assert not [s for s in body[: first("v_mfma")] if s.startswith("s_barrier")]
    assert not [s for s in body[: first("global_load_dwordx4")] if re.match(r"(global|buffer|flat|scratch)_load", s)]


def test_records_kernel_is_one_load_and_fold(frames_co):
    """frame_records_kernel keeps frame_record_kernel's shape (tests/test_crc_isa.py): every load is issued before the first wait on
    vector memory."""
    body = kernel_text(frames_co, "_ZN2t320frame_records_kernel")
    loads = [i for i, s in enumerate(body) if s.startswith("global_load")]
    waits = [i for i, s in enumerate(body) if s.startswith("s_waitcnt") and "vmcnt" in s]
    assert loads and waits and max(loads) < min(waits)
    assert sum(1 for s in body if s.startswith("s_waitcnt") and "vmcnt(0)" in s) <= 2


def test_new_object_carries_no_compiler_crc_table(frames_co):
    syms = symbols(frames_co)
    assert syms and not [s for s in syms if s.startswith(".crctable")]
