"""CPU proof of the erasure repair's yardstick (tests/erasure_patterns.py) and of the errors-and-erasures block decoder itself, through
t3hip_rs_decode_block_erasures_host -- the same t3_rs_core.h code the kernels run --, and the host-only part of the new entries: the
argument checks and the built kernels.

The rule (include/t3hip.h, "repair with erasures"): bytes above 26 are erasures, s of them; a block is accepted iff a codeword c exists
with 2 e + s <= r, e = the other positions where c differs from the received symbol; accepted -> c, refused -> untouched."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import erasure_patterns as ep
import oracle_lib as ol
import rs_patterns as rp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = (24, 22, 20, 18)
E_ARG = -3
REPS = 20                                                                 # constructed cases per (s, e)
BEYOND_REPS = {24: 40, 22: 40, 20: 30, 18: 20}                            # per pair; the s = 0 rows of k = 20, 18 walk all 2 952 / 17 902 subsets


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    return ge.load_package()


@functools.lru_cache(maxsize=None)
def constructed_pool(k):
    src = ep.ByteSource()
    return ep.block_pool(ol.oracle(), k, ep.admissible(k) * REPS, 20261020, src) + (src,)


@functools.lru_cache(maxsize=None)
def beyond_pool(k):
    return ep.block_pool(ol.oracle(), k, ep.beyond(k) * BEYOND_REPS[k], 20261021)


def host_decode(t3, k, rec):
    """-> (ok (n,), the blocks afterwards (n, 26), data rows of the accepted blocks)"""
    ok = np.zeros(len(rec), bool); out = np.zeros_like(rec); data = {}
    for i, r in enumerate(rec):
        ok[i], out[i], d = t3.rs_decode_block_erasures_host(k, r)
        if ok[i]:
            data[i] = d
    return ok, out, data


# ---- 1. the yardstick with s = 0 is the oracle's FIXED block decoder ---------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
def test_yardstick_without_erasures_is_the_oracle(orc, k):
    Y = ep.yardstick(orc); t = rp.tparam(k)
    rows, wt = rp.canonical(k, 0)
    pick = np.concatenate([np.flatnonzero(wt == w)[:: max(1, int((wt == w).sum()) // 12)][:14] for w in range(t + 1)])   # every weight 0..t
    near, far = rp.near_errors(k), rp.far_errors(k)
    n_far = 40 if k >= 22 else 14
    y = np.concatenate([rows[pick], near[:: max(1, len(near) // 20)][:20], far[:n_far // 2], far[52: 52 + n_far // 2]])
    assert set(wt[pick].tolist()) == set(range(t + 1))
    cw, _, ok = orc.rs_decode_blocks(k, y, mode=1)
    got_ok, got_cw = Y.decide_rows(k, y, np.zeros_like(y, bool))
    assert np.array_equal(got_ok, ok == 1), k
    assert got_ok[: len(pick) + 20].all() and not got_ok[len(pick) + 20:].any(), k        # schedule and near rows accepted, far rows refused
    assert np.array_equal(got_cw[got_ok], cw[got_ok]), k


# ---- 2. every (s, e) with 2 e + s <= r ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
def test_constructed_blocks_within_capacity(built, orc, k):
    clean, rec, mask, err, _ = constructed_pool(k)
    pairs = ep.admissible(k) * REPS
    assert sorted(set(pairs)) == sorted((s, e) for s in range(26 - k + 1) for e in range(27) if 2 * e + s <= 26 - k)
    assert np.array_equal(mask.sum(axis=1), [s for s, _ in pairs]) and np.array_equal((err != 0).sum(axis=1), [e for _, e in pairs])
    assert np.array_equal(rec > 26, mask) and not (err != 0)[mask].any()
    ok, out, data = host_decode(built, k, rec)
    assert ok.all(), (k, [pairs[i] for i in np.flatnonzero(~ok)][:5])
    assert np.array_equal(out, clean), k
    assert all(np.array_equal(data[i], clean[i, :k]) for i in range(len(rec))), k
    yok, ycw = ep.yardstick(orc).decide_rows(k, rec % 27, mask)
    assert yok.all() and np.array_equal(ycw, clean), k


def test_erased_bytes_cover_every_value():
    """27..255 at erased positions over the constructed set, residues both right and wrong"""
    for k in KS:
        src = constructed_pool(k)[4]
        assert src.right > 0 and src.wrong > 0, k
    _, rec, mask, _, src = constructed_pool(18)
    assert src.seen == set(range(27, 256)) == set(rec[mask].tolist())


# ---- 3. beyond capacity -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
def test_beyond_capacity_matches_the_yardstick(built, orc, k):
    r = 26 - k
    clean, rec, mask, err = beyond_pool(k)
    pairs = ep.beyond(k) * BEYOND_REPS[k]
    assert {2 * e + s for s, e in pairs if s <= r} == {r + 1, r + 2} and {s for s, e in pairs if s > r} >= {r + 1, 26}
    ok, out, data = host_decode(built, k, rec)
    yok, ycw = ep.yardstick(orc).decide_rows(k, rec % 27, mask)
    assert np.array_equal(ok, yok), (k, [pairs[i] for i in np.flatnonzero(ok != yok)][:5])
    assert np.array_equal(out[~ok], rec[~ok]), k                                        # refused: untouched
    assert not ok[mask.sum(axis=1) > r].any(), k
    acc = np.flatnonzero(ok)
    assert np.array_equal(out[acc], ycw[acc]), k                                         # a miscorrection is the yardstick's too
    assert rp.is_codeword(orc, k, out[acc]).all()
    outside = ((out[acc] != rec[acc]) & ~mask[acc]).sum(axis=1)
    assert (2 * outside + mask[acc].sum(axis=1) <= r).all(), k
    assert all(np.array_equal(data[i], out[i, :k]) for i in acc)
    assert not ok.all()                                                                  # (most of the pool is refused)


# ---- 4. the documented difference to the plain rule -----------------------------------------------------------------------------------------
def test_flagged_byte_with_the_right_residue(built, orc):
    """RS(26,24), one flagged byte whose residue is right, one error elsewhere: 2 * 1 + 1 > 2.  The errors-only decoder takes the byte
    mod 27, sees one error and accepts; the erasure rule does not trust the byte and refuses."""
    F = rp.field(orc)
    rng = np.random.default_rng(24)
    clean = orc.rs_encode_blocks(24, rng.integers(0, 27, (26, 24)).astype(np.uint8), mode=1)
    for i, c in enumerate(clean):
        rec = c.copy()
        p, q = i, (i + 7) % 26
        rec[p] = c[p] + 27 * (1 + i % 8)
        rec[q] = F.add[c[q], 1 + i % 26]
        ok, out, _ = built.rs_decode_block_erasures_host(24, rec)
        assert not ok and np.array_equal(out, rec), i
        assert ep.yardstick(orc).decide(24, rec % 27, rec > 26)[0] is False
        good, cw = _plain_host(built, rec)
        assert good and np.array_equal(cw, c), i
        rec[q] = c[q]                                                                    # without the error: s = 1 <= 2
        ok, out, d = built.rs_decode_block_erasures_host(24, rec)
        assert ok and np.array_equal(out, c) and np.array_equal(d, c[:24]), i


def _plain_host(t3, rec):
    import ctypes as C
    c = np.ascontiguousarray(rec, np.uint8).copy(); d = np.zeros(24, np.uint8)
    rc = t3.lib().t3hip_rs_decode_block_host(C.c_int(24), C.c_int(1), c.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p))
    return rc == 1, c


def test_host_entry_arguments(built):
    import ctypes as C
    L = built.lib()
    buf = (C.c_uint8 * 26)(); d = (C.c_uint8 * 26)()
    assert L.t3hip_rs_decode_block_erasures_host(C.c_int(19), buf, d) == E_ARG
    assert L.t3hip_rs_decode_block_erasures_host(C.c_int(20), None, d) == E_ARG
    assert L.t3hip_rs_decode_block_erasures_host(C.c_int(20), buf, None) == E_ARG
    assert L.t3hip_rs_decode_block_erasures_host(C.c_int(20), buf, d) == 1             # the zero word


# ---- 5. arguments, then the stream, then the device -----------------------------------------------------------------------------------------
NODEV = r"""
import ctypes as C, sys
sys.path.insert(0, %r)
import __graft_entry__ as ge
t3 = ge.load_package()
L = t3.lib()
assert not t3.is_ready()
cfg = t3.make_cfg(profile=2, uep=2, mode=1); compat = t3.make_cfg(profile=2, uep=2, mode=0); raw = t3.make_cfg(profile=0xFF, mode=1)
n_raw = 64; n_in = int(t3.plan(n_raw, cfg).out_words)
buf = (C.c_uint8 * (9 * n_in + 16))(); ver = (C.c_uint32 * 6)(); cnt = (C.c_uint32 * 6)()
base = C.addressof(buf); base += base & 1
def run(io=base, n=n_in, c=cfg, flags=1, v=C.addressof(ver)):
    return L.t3hip_repair_erasures_frame_async(C.c_void_p(io), C.c_uint64(n), C.byref(c) if c is not None else None, C.c_uint64(n_raw), C.c_uint32(flags), C.c_void_p(v), None)
E_ARG, E_HEADER = -3, -5
assert run(c=None) == E_ARG and run(v=None) == E_ARG and run(io=None) == E_ARG and run(io=base + 1) == E_ARG and run(flags=2) == E_ARG
assert run(c=compat) == E_ARG and run(c=raw) == E_ARG
assert run(n=n_in - 1) == E_HEADER and run(n=n_in - 1, flags=2) == E_ARG
assert run() == t3.E_NODEVICE and run(flags=0) == t3.E_NODEVICE and run(io=base + 2) == t3.E_NODEVICE
seen = t3.DecoderContext(mode=1).cfg_last_seen
for fn, tail in ((L.t3hip_repair_erasures_profile_dev, (None,)), (L.t3hip_repair_erasures_profile, ())):
    assert fn(C.c_void_p(base), C.c_uint64(n_in), C.byref(compat), C.c_uint32(1), cnt, *tail) == E_ARG
    assert fn(C.c_void_p(base), C.c_uint64(n_in), C.byref(raw), C.c_uint32(1), cnt, *tail) == E_ARG
    assert fn(C.c_void_p(base), C.c_uint64(n_in), C.byref(seen), C.c_uint32(1), None, *tail) == E_ARG
    assert fn(C.c_void_p(base), C.c_uint64(n_in), C.byref(seen), C.c_uint32(2), cnt, *tail) == E_ARG
    assert fn(C.c_void_p(base), C.c_uint64(n_in), C.byref(seen), C.c_uint32(1), cnt, *tail) == t3.E_NODEVICE
code = (C.c_uint8 * 52)(); data = (C.c_uint8 * 52)(); ok = (C.c_uint8 * 2)()
for fn, tail in ((L.t3hip_rs_decode_blocks_erasures_dev, (None,)), (L.t3hip_rs_decode_blocks_erasures, ())):
    assert fn(C.c_int(21), code, C.c_uint64(2), data, ok, *tail) == E_ARG
    assert fn(C.c_int(20), None, C.c_uint64(2), data, ok, *tail) == E_ARG
    assert fn(C.c_int(20), code, C.c_uint64(2), None, ok, *tail) == E_ARG
    assert fn(C.c_int(20), code, C.c_uint64(2), data, None, *tail) == E_ARG
    assert fn(C.c_int(20), code, C.c_uint64(2), data, ok, *tail) == t3.E_NODEVICE
assert t3.repair_plan(n_raw, cfg).path == 1
print("ok")
"""


def test_arguments_then_the_device(built):
    """A process that never initialised a device: every bad argument is refused before the entries ask for one, a truncated stream after
    the arguments, and only then T3_E_NODEVICE (no CPU fallback).  (The addresses are host memory and never read: no device, no launch.)"""
    r = subprocess.run([sys.executable, "-c", NODEV % ROOT], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


# ---- 6. the built objects -------------------------------------------------------------------------------------------------------------------
def test_kernels_built_once(built):
    """The new kernels exist exactly once each, and their names hide no older kernel from the tests that count those by substring."""
    sys.path.insert(0, os.path.join(ROOT, "profiles"))
    import kernel_resources as kr
    ks = kr.all_kernels()
    for r in (2, 4, 6, 8):
        assert len([n for n in ks if "erasure_fixed_kernel<%d>" % r in n]) == 1, r
        assert len([n for n in ks if "repair_fixed_kernel<%d>" % r in n]) == 1, r
        assert len([n for n in ks if "repair_frames_kernel<%d>" % r in n]) == 1, r
    for name in ("erasure_generic_kernel", "rs_erasure_blocks_kernel", "repair_generic_kernel", "hdr_compare_frames_kernel", "rs_decode_blocks_kernel",
                 "crc_fp4_kernel", "frame_record_kernel", "frame_records_kernel", "crc_fp4_frames_kernel", "image_compose_frames_kernel"):
        assert len([n for n in ks if name + "(" in n or name + "<" in n]) >= 1, name
    for name in ("erasure_generic_kernel", "rs_erasure_blocks_kernel", "repair_generic_kernel", "hdr_compare_frames_kernel"):
        assert len([n for n in ks if name in n]) == 1, name
    era = set(kr.kernel_notes(os.path.join(kr.CSRC, "t3_repair_era.o")))
    assert len(era) == 6, sorted(era)
    # the fused kernel: two 8-wave workgroups per CU (128 VGPRs), nothing spilled, no scratch access inside the tile loop
    loops = kr.loop_scratch(["t3_repair_era.o"])
    for r in (2, 4, 6, 8):
        name = [n for n in ks if "erasure_fixed_kernel<%d>" % r in n][0]
        assert int(ks[name]["vgpr_spill_count"]) == 0 and int(ks[name]["vgpr_count"]) <= 128, (name, ks[name])
        assert loops[name] == (0, 0), (name, loops[name])
