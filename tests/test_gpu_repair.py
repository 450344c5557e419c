"""GPU tests of the FIXED stream repair (include/t3hip.h, "repair"): repair_fixed_kernel<R> (one k on all bands, no beacon, 1-D and the
64 x 64 2-D frame) and repair_generic_kernel (beacon, per-band k, four codes, 7 x 5 tiles) against the yardstick of
tests/test_repair_semantics.py -- expected(received), built from rs_patterns and the oracle only and proven there on the CPU.  The buffer
after a repair equals expected byte for byte, the four verdict words are the yardstick's, and the bytes in front of and behind the frame's
9 * n_in bytes are untouched (tests/bounds.py).  Byte work: every comparison is exact."""
import functools
import json
import os
import subprocess

import numpy as np
import pytest

import bounds
import oracle_lib as ol
import rs_patterns as rp
from test_repair_semantics import FUSED, GENERIC, SIZES, SWEEP, expected

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = bounds.FILLS[0]


@functools.lru_cache(maxsize=4)
def _frame(name, what):
    import __graft_entry__ as ge
    t3 = ge.load_package()
    cfg = t3.make_cfg(mode=1, **rp.CONFIGS[name])
    return rp.make_frame(ol.oracle(), lambda n_raw: t3.plan(n_raw, cfg), name, what)


def run(gpu, fr, stream, flags, offset=0, fill=FILL):
    """One t3hip_repair_frame_async on a guarded copy of `stream` -> (the frame's bytes afterwards, the four words); the guards are
    checked, every byte of the frame may change."""
    import torch
    b = np.ascontiguousarray(stream, np.uint8).reshape(-1)
    buf = bounds.Buf(len(b), fill, offset, data=b, name="frame", may_change=((0, len(b)),))
    ver = torch.full((4,), 7, dtype=torch.int32, device="cuda")
    cfg = gpu.make_cfg(mode=1, **fr.kw)
    gpu.repair_frame_async(buf.ptr, len(b) // 9, cfg, fr.n_raw, flags, ver.data_ptr(), torch.cuda.current_stream().cuda_stream)
    bounds.sync()
    return buf.result(), ver.cpu().tolist()


def check_case(gpu, orc, fr, s, tag, offset=0, dry=True, again=True):
    exp, words, _ = expected(orc, fr, s)
    rec = np.ascontiguousarray(s).reshape(-1)
    got, ver = run(gpu, fr, s, gpu.REPAIR_WRITE, offset)
    assert ver == [0] + words, (tag, "words", ver, words)
    bounds.check_equal(got, exp, FILL, "repaired %s" % (tag,))
    if dry:                                                                # the same words, no byte stored
        got, ver = run(gpu, fr, s, 0, offset)
        assert ver == [0] + words, (tag, "dry run", ver, words)
        assert np.array_equal(got, rec), (tag, "dry run wrote")
    if again:                                                              # a repair of the repaired frame: nothing left to change
        got, ver = run(gpu, fr, exp, gpu.REPAIR_WRITE, offset)
        assert ver == [0, words[0], 0, 0], (tag, "second repair", ver)
        assert np.array_equal(got, exp), (tag, "second repair wrote")
    return exp, words


# ---- the main sweep ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", SIZES)
@pytest.mark.parametrize("name", SWEEP)
def test_repair_sweep(gpu, orc, name, what):
    """Every framing at three sizes, the CASES of each size: buffer = expected, words = the yardstick's, guards untouched."""
    fr = _frame(name, what)
    assert gpu.repair_plan(fr.n_raw, gpu.make_cfg(mode=1, **fr.kw)).path == (1 if name in FUSED else 0)
    for case in rp.CASES[what]:
        s, M, _ = fr.stream(case)
        _, words = check_case(gpu, orc, fr, s, (name, what, case), dry=False, again=False)
        assert words[0] == M
    got, ver = run(gpu, fr, fr.clean, gpu.REPAIR_WRITE)                    # a clean canonical frame is a fixed point
    assert ver == [0, 0, 0, 0] and np.array_equal(got, fr.clean.reshape(-1)), (name, what, "clean")


@pytest.mark.parametrize("what", ("small", "padded"))
@pytest.mark.parametrize("name", SWEEP)
def test_dry_run_and_second_repair(gpu, orc, name, what):
    """Without T3_REPAIR_WRITE: the same words, the buffer unchanged.  A repair of the repaired buffer: words [2] = [3] = 0, unchanged."""
    fr = _frame(name, what)
    for case in rp.CASES[what]:
        check_case(gpu, orc, fr, fr.stream(case)[0], (name, what, case))


# ---- bytes 27..255 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("k20", "k20_beacon83"))
def test_noncanonical_bytes(gpu, orc, name):
    """The LIFTS patterns of `full`: an accepted block comes back canonical, in a far block the lifted bytes stay, a beacon slot gets the
    encoder's symbol whatever it held."""
    fr = _frame(name, "full")
    for base, pattern in rp.lift_names(fr, "full"):
        s, _, M, where = rp.lifted(fr, base, pattern)
        assert (s > 26).any()
        exp, words = check_case(gpu, orc, fr, s, (name, base, pattern), dry=pattern == "dense", again=False)
        assert words[0] == M and words[2] >= int((s > 26).sum()) - 26 * M
        B = rp.block_index(fr.L, fr.ocfg); f0 = rp.band_first_block(fr.L)
        far_rows = [f0[b] + m for (b, m) in where]
        keep = np.ones(len(exp), bool); keep[B[far_rows].reshape(-1)] = False
        assert exp[keep].max() <= 26
        if M:
            assert (exp[B[far_rows]] > 26).any() and np.array_equal(exp[B[far_rows]], s.reshape(-1)[B[far_rows]])


# ---- base address -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("k20", "k18", "luma"))
def test_base_address_2_mod_16(gpu, orc, name):
    fr = _frame(name, "padded")
    for fill in bounds.FILLS:
        for case in rp.CASES["padded"]:
            s = fr.stream(case)[0]
            exp, words, _ = expected(orc, fr, s)
            got, ver = run(gpu, fr, s, gpu.REPAIR_WRITE, offset=2, fill=fill)
            assert ver == [0] + words, (name, case, fill)
            bounds.check_equal(got, exp, fill, "repaired at 2 mod 16")


# ---- the tile loop ----------------------------------------------------------------------------------------------------------------------
def test_tile_loop(gpu, orc):
    """One k20 frame of at least 3 x (3 x CU count) fused tiles, so that every workgroup walks its loop more than twice; the <= t
    schedule in every band (the body of a one-k frame without beacon is one run of 26-byte blocks)."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    tiles = 9 * cus + 1
    n_px = tiles * 108 * 20 - 1001                                          # the last tile ragged, the count odd
    cfg = gpu.make_cfg(mode=1, **rp.CONFIGS["k20"])
    fr = rp.Frame(orc, lambda n_raw: gpu.plan(n_raw, cfg), "k20", n_px, 103)
    p = gpu.repair_plan(fr.n_raw, cfg)
    assert p.path == 1 and p.n_tiles >= 3 * 3 * cus and p.blocks_per_tile == 9 * 52
    s, rec = fr.sched()
    for b in range(9):
        rp.assert_coverage(20, rec[b])
    flat, clean = s.reshape(-1), fr.clean.reshape(-1)
    hs, nb = int(fr.L.header_syms), int(fr.L.body_syms)
    diff = (flat != clean)[hs: hs + nb].reshape(-1, 26)
    assert not (flat != clean)[:hs].any() and not (flat != clean)[hs + nb:].any()
    words = [0, 0, int(diff.any(axis=1).sum()), int(diff.sum())]
    got, ver = run(gpu, fr, s, gpu.REPAIR_WRITE)
    assert ver == words, (ver, words)
    bounds.check_equal(got, clean, FILL, "tile loop")


# ---- the synchronous entries ------------------------------------------------------------------------------------------------------------
def _damage_header(stream, n):
    """n symbol errors in the header's first RS(26,18) block (t = 4)"""
    s = np.ascontiguousarray(stream, np.uint8).copy().reshape(-1)
    at = np.arange(n) * 2 + 1
    s[at] = (s[at] + 1 + np.arange(n) % 25) % 27
    return s


@pytest.mark.parametrize("name", ("k20", "k20_beacon83"))
def test_profile_entries(gpu, orc, name):
    import torch
    fr = _frame(name, "padded")
    cfg = gpu.make_cfg(mode=1, **fr.kw)
    hdr = gpu.header_encode(cfg, fr.n_raw)
    assert np.array_equal(fr.clean.reshape(-1)[: len(hdr)], hdr)
    n_in = len(fr.clean)
    sched = fr.stream("sched")[0]
    far, M, where = fr.stream("far2")
    cases = (("header+2", _damage_header(sched, 2), gpu.OK, True), ("header+9", _damage_header(sched, 9), gpu.E_HEADER, False),
             ("far2", np.ascontiguousarray(far).reshape(-1), gpu.E_RS, False))
    for label, s, want_rc, hdr_fixed in cases:
        exp, words, _ = expected(orc, fr, s)
        if hdr_fixed:
            exp = exp.copy(); exp[: len(hdr)] = hdr                          # ... and the header comes back as t3hip_header_encode's bytes
        if want_rc == gpu.E_HEADER:
            exp, words = s, [0, 0, 0]                                        # nothing written
        for flags in (gpu.REPAIR_WRITE, 0):
            tag = (name, label, flags)
            buf = bounds.Buf(len(s), FILL, 0, data=s, name="frame", may_change=((0, len(s)),))
            rc, counts = gpu.repair_profile_dev(buf.ptr, n_in, gpu.DecoderContext(mode=1).cfg_last_seen, flags, torch.cuda.current_stream().cuda_stream)
            bounds.sync()
            assert rc == want_rc and counts == [1 if hdr_fixed else 0] + words, (tag, rc, counts, words)
            bounds.check_equal(buf.result(), exp if flags else s, FILL, "profile_dev %s" % (tag,))
            w = s.copy().reshape(-1, 9)
            rc, counts = gpu.repair_profile(w, gpu.DecoderContext(mode=1), flags)
            assert rc == want_rc and counts == [1 if hdr_fixed else 0] + words, (tag, "host", rc, counts)
            assert np.array_equal(w.reshape(-1), exp if flags else s), (tag, "host")
    with pytest.raises(gpu.T3Error) as e:                                     # seen->mode must be FIXED on entry
        gpu.repair_profile(sched.copy(), gpu.DecoderContext(mode=0))
    assert e.value.code == gpu.E_ARG


def test_repair_demo(gpu, orc, tmp_path):
    """tests/cpp/repair_demo.cpp: a relay's loop through repair_profile of include/ternary_codec_v6.hpp, built with g++ alone."""
    lib = os.path.join(ROOT, "ternary-image-codec_amd")
    exe = str(tmp_path / "repair_demo")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "repair_demo.cpp"),
                    "-L" + lib, "-lt3hip", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-o", exe], check=True)
    fr = _frame("k20", "padded")
    hdr_len = int(fr.L.header_syms)
    for case, hdr_errors in (("sched", 2), ("far2", 0)):
        s, M, _ = fr.stream(case)
        s = _damage_header(s, hdr_errors)
        exp, words, _ = expected(orc, fr, s)
        exp = exp.copy(); exp[:hdr_len] = fr.clean.reshape(-1)[:hdr_len]
        fin, fout = str(tmp_path / "in.words"), str(tmp_path / "out.words")
        s.tofile(fin)
        out = json.loads(subprocess.run([exe, fin, fout], check=True, capture_output=True, text=True).stdout)
        assert out == {"ok": 0 if M else 1, "status": gpu.E_RS if M else 0, "header_rewritten": 1 if hdr_errors else 0, "uncorrectable": M,
                       "blocks_changed": words[1], "bytes_changed": words[2]}, (case, out)
        assert np.array_equal(np.fromfile(fout, np.uint8), exp), case


# ---- cross-check with the decoder -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("k20", "k18"))
def test_decoder_on_the_repaired_buffer(gpu, orc, name):
    """t3hip_decode_frame_async of the repaired buffer: the pixels of the clean frame outside the far tiles, verdict [0, M]."""
    import torch
    fr = _frame(name, "full")
    cfg = gpu.make_cfg(mode=1, **fr.kw)
    n = len(fr.padded); st = torch.cuda.current_stream().cuda_stream
    for case in ("sched", "near", "far1000"):
        s, M, where = fr.stream(case)
        d = torch.from_numpy(np.ascontiguousarray(s).reshape(-1).copy()).cuda()
        ver4 = torch.full((4,), 7, dtype=torch.int32, device="cuda"); ver = torch.full((2,), 7, dtype=torch.int32, device="cuda")
        out = torch.full((6 * n + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        gpu.repair_frame_async(d.data_ptr(), d.numel() // 9, cfg, fr.n_raw, gpu.REPAIR_WRITE, ver4.data_ptr(), st)
        got = gpu.decode_frame_async(d.data_ptr(), d.numel() // 9, cfg, fr.n_raw, out.data_ptr(), n, ver.data_ptr(), True, st)
        bounds.sync()
        assert got == n and ver.cpu().tolist() == [0, M] and ver4.cpu().tolist()[:2] == [0, M], (name, case)
        px = out[: 6 * n].cpu().numpy().view(ol.PIXEL_DT)
        if case == "near":
            rc, want = orc.decode_frame(s, ol.make_cfg(mode=1))
            assert rc == 0 and np.array_equal(px, want), (name, case)
        else:
            keep = rp.pixels_outside_tiles(n, fr.ks[0], rp.far_tiles_one_k(fr.ks[0], where))
            assert keep.any() and np.array_equal(px[keep], fr.padded[keep]), (name, case)
