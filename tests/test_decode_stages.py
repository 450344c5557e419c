"""The reference decoder's stages one at a time (OLD:918-993: read_and_decode_header_from_words, descramble_words_inplace,
demap_and_rsdecode_bands_from_words) and its single-word subword helpers (OLD:816-833), against the oracle.  The oracle's
scramble, rs_decode_blocks and decode_profile are pinned to the unmodified reference on decoder-consistent streams by
test_oracle_vs_ref.py, so what is pinned to them here is pinned to the reference transitively.

The yardstick of stage 3 is the numpy restatement of OLD:948-993 (restate_stage3, in tests/stage_shapes.py, which the workgroup-step tests
of tests/test_gpu_stage_steps.py share); test_restatement_composes_to_decode_profile
checks it first: composed with the header read, the descramble, the de-interleave and the trit regroup it must reproduce the oracle's
decode_profile_to_raw, verdict, words and cfg_last_seen."""
import json
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

import oracle_lib as ol
from oracle_lib import make_cfg
from stage_shapes import CODESETS, KS, UEPS, band_columns, band_offsets, restate_stage3, stage_body  # noqa: F401 (shared with the step tests)
from test_oracle_vs_ref import CFGS, decoder_consistent_stream

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (0, 1, 25, 26, 27, 130, 600)
N8K = 20_766_720                                   # body words of an 8K frame at RS(26,20): 798,720 blocks per band

STAGE_CFGS = dict(CFGS)
STAGE_CFGS["p2_beacon_period1"] = dict(profile=1, uep=1, beacon=(1, 4, 1))   # period 1: the beacon band is empty


# ---- the restatement (stage 3: stage_shapes.restate_stage3) --------------------------------------------------------------
def restate_header(orc, words, cursor, mode=0):
    """OLD:918-937 -> (ok, cursor, header_unpack tuple or None)."""
    w = np.asarray(words, np.uint8).reshape(-1, 9)
    if cursor + 6 > len(w):
        return False, cursor, None
    sy = w[cursor: cursor + 6].reshape(-1)
    cursor += 6
    _, dk, okv = orc.rs_decode_blocks(18, np.stack([sy[:26], sy[26:52]]), mode=mode)
    if not (okv[0] and okv[1]):
        return False, cursor, None
    hp = np.concatenate([dk[0], dk[1][:9]])
    if not orc.header_check(hp):
        return False, cursor, None
    return True, cursor, orc.header_unpack(hp)


SEEN_FIELDS = ("profile", "tile_w", "tile_h", "seed_a", "seed_b", "seed_s0", "beacon_words_period", "beacon_band_slot", "beacon_enabled",
               "subword", "centered", "coset")


def regroup_words(use):
    """symbols -> trits -> 26 trits per word, T[26] = 0 (OLD:1022-1040)."""
    tr = np.stack([use % 3, use // 3 % 3, use // 9 % 3], 1).reshape(-1)
    n = len(tr) // 26
    T = np.zeros((n, 27), np.uint8)
    T[:, :26] = tr[: 26 * n].reshape(n, 26)
    return (T[:, 0::3] + 3 * T[:, 1::3] + 9 * T[:, 2::3]).astype(np.uint8)


def restate_decode_profile(orc, stream):
    """decode_profile_to_raw (OLD:995-1041) from the restated stages -> (ok, words, cfg_last_seen)."""
    seen = make_cfg()
    ok, cur, hu = restate_header(orc, stream, 0)
    if not ok:
        return False, np.zeros((0, 9), np.uint8), seen
    h = hu[0]
    for f in SEEN_FIELDS:
        setattr(seen, f, getattr(h, f))
    for i in range(9):
        seen.band_profile[i] = h.band_profile[i]
    body = orc.scramble(np.asarray(stream, np.uint8).reshape(-1, 9)[cur:].reshape(-1), h.seed_a, h.seed_b, h.seed_s0, 1)
    ok, use = restate_stage3(orc, body, h)
    if not ok:
        return False, np.zeros((0, 9), np.uint8), seen
    if h.profile == 4 and h.tile_w and h.tile_h:
        use = orc.interleave2d(use, h.tile_w, h.tile_h, 1)
    return True, regroup_words(use), seen


def stage_streams(orc, name):
    """(stream, header cfg) of every size and corruption level of test 1, decoder-consistent (test_oracle_vs_ref.decoder_consistent_stream)."""
    rng = np.random.default_rng(zlib.crc32(name.encode()) + 7)
    cfg = make_cfg(**STAGE_CFGS[name])
    for nbw in SIZES:
        for corrupt in (0, 1, 5):
            yield nbw, corrupt, decoder_consistent_stream(orc, rng, cfg, nbw, corrupt)


# ---- 1. the yardstick ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(STAGE_CFGS))
def test_restatement_composes_to_decode_profile(orc, name):
    for nbw, corrupt, s in stage_streams(orc, name):
        sa = make_cfg()
        ra, a = orc.decode_profile(s, sa)
        ok, words, seen = restate_decode_profile(orc, s)
        assert (ra == 0) == ok, (name, nbw, corrupt)
        assert np.array_equal(a, words), (name, nbw, corrupt)
        assert sa.as_dict() == seen.as_dict(), (name, nbw, corrupt)
        if corrupt == 0:
            assert ok


# ---- 2. the reference names compile; their host part runs without a device ----------------------------------------------------
def build_stage_demo(tmp):
    exe = os.path.join(tmp, "stage_names_demo")
    lib = os.path.join(ROOT, "ternary-image-codec_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include", "compat"), "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "stage_names_demo.cpp"), "-L" + lib, "-lt3hip", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib",
                    "-o", exe], check=True)
    return exe


def header_words(orc, cfg, mode_parity=1, errors=(0, 0), rng=None):
    """Six header words: blocks A / B = RS(26,18) codewords (FIXED parity) of header_pack(cfg), errors[q] symbol errors in block q."""
    hp = orc.header_pack(cfg, 1234, 567)
    A = orc.rs_encode_blocks(18, hp[:18], mode=mode_parity)[0]
    B = orc.rs_encode_blocks(18, np.concatenate([hp[18:], np.zeros(9, np.uint8)]), mode=mode_parity)[0]
    for blk, e in zip((A, B), errors):
        if e:
            pos = rng.choice(26, size=e, replace=False)
            blk[pos] = (blk[pos] + rng.integers(1, 27, e)) % 27
    return np.concatenate([A, B, np.zeros(2, np.uint8)]).reshape(6, 9)


def host_cases(orc):
    rng = np.random.default_rng(31)
    words = rng.integers(0, 256, size=(40, 9), dtype=np.uint8)              # non-canonical symbols too
    words[:8] = rng.integers(0, 27, size=(8, 9), dtype=np.uint8)
    inject = []
    for N in (0, 1, 15, 26, 27, 30):
        for fill in (0, 1, 2):
            inject.append((N, fill, rng.integers(0, 3, 30, dtype=np.uint8)))
            inject.append((N, fill, rng.integers(0, 7, 30, dtype=np.uint8)))     # out-of-range trits pass through
    hdrs = []
    for cname in ("p2_luma", "p5_tile7x5_mixed", "p1_beacon_small", "p4_seed_wrap"):
        cfg = make_cfg(**CFGS[cname])
        for mode in (0, 1):
            good = header_words(orc, cfg)
            hdrs.append((good, 0, mode))                                         # a good header
            hdrs.append((np.concatenate([rng.integers(0, 27, (5, 9), dtype=np.uint8), good, good[:3]]), 5, mode))   # cursor in the middle
            for e in (1, 2, 4):
                hdrs.append((header_words(orc, cfg, errors=(e, e), rng=rng), 0, mode))     # <= 4 symbol errors per block
            hdrs.append((header_words(orc, cfg, errors=(9, 0), rng=rng), 0, mode))         # uncorrectable
            hdrs.append((good[:5], 0, mode))                                     # shorter than six words
            hdrs.append((good, 1, mode))                                         # fewer than six words behind the cursor
    return words, inject, hdrs


def write_host_cases(path, words, inject, hdrs):
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(words))); f.write(np.ascontiguousarray(words).tobytes())
        f.write(struct.pack("<I", len(inject)))
        for N, fill, t in inject:
            f.write(struct.pack("<iB", N, fill)); f.write(t.tobytes())
        f.write(struct.pack("<I", len(hdrs)))
        for w, cur, mode in hdrs:
            f.write(struct.pack("<IQB", len(w), cur, mode)); f.write(np.ascontiguousarray(w, np.uint8).tobytes())


def test_stage_names_host_part(orc, tmp_path):
    """tests/cpp/stage_names_demo.cpp compiles against include/compat (all five reference names) and its host part -- the word helpers and
    the header read, which are host arithmetic -- runs without a device; every value against the oracle and the restatement."""
    exe = build_stage_demo(str(tmp_path))
    words, inject, hdrs = host_cases(orc)
    path = os.path.join(str(tmp_path), "host.bin")
    write_host_cases(path, words, inject, hdrs)
    out = json.loads(subprocess.run([exe, "host", path], check=True, capture_output=True, text=True).stdout)
    for w, got in zip(words, out["extract"]):                                 # all 27 trits, whatever N
        assert got == list(orc.extract_subword_stream(w, 27))
    assert len(out["extract"]) == len(words)
    for (N, fill, t), got in zip(inject, out["inject"]):
        n = min(max(N, 0), 27)
        T = np.concatenate([t[:n], np.full(27 - n, fill, np.uint8)]).astype(np.int64)
        want = list(T[0::3] + 3 * T[1::3] + 9 * T[2::3])                     # pack3, no reduction
        assert got == want, (N, fill)
        if t.max() < 3 and 1 <= N <= 27:
            assert got == list(orc.build_words_from_subword_stream(t[:N], N, fill)[0])
    assert len(out["inject"]) == len(inject)
    n_ok = 0
    for (w, cur, mode), got in zip(hdrs, out["header"]):
        ok, cur2, hu = restate_header(orc, w, cur, mode)
        assert got["ok"] == int(ok) and got["cursor"] == cur2, (cur, mode, len(w))
        if ok:
            n_ok += 1
            c, fs, bh, mg, ver = hu
            assert (got["frame_seq"], got["band_map_hash"], got["magic"], got["version"]) == (fs, bh, mg, ver)
            h = got["hdr"]
            assert h["band_profile"] == list(c.band_profile) and all(h[f] == getattr(c, f) for f in SEEN_FIELDS)
        else:
            assert got["frame_seq"] == 4242                                   # `out` untouched on a false
    assert len(out["header"]) == len(hdrs) and 0 < n_ok < len(hdrs)


# ---- 3. register budget --------------------------------------------------------------------------------------------------
def test_stage_kernels_no_spills_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "profiles"))
    import kernel_resources
    ks = {n: v for n, v in kernel_resources.all_kernels().items() if "descramble_words_kernel" in n or "stage_decode_kernel" in n}
    assert len(ks) >= 2, sorted(ks)
    for n, v in ks.items():
        assert int(v["vgpr_spill_count"]) == 0 and int(v["private_segment_fixed_size"]) == 0, (n, v)


# ---- GPU -------------------------------------------------------------------------------------------------------------------
def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.uint8).reshape(-1).copy()).cuda()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 2, 3, 7, 1000, N8K])
def test_descramble_words_dev(gpu, orc, n):
    import torch
    t3 = gpu
    rng = np.random.default_rng(n + 5)
    words = rng.integers(0, 256, 9 * n, dtype=np.uint8)
    for off in (0, 1, 54, 90):
        buf = rng.integers(0, 256, off + 9 * n + 37, dtype=np.uint8)
        buf[off: off + 9 * n] = words
        for seed in ((1, 1, 1), (2, 1, 0), (0, 0, 0), (0xFFFFFFFF, 0xFFFFFFFE, 5)):
            d = _dev(buf)
            t3.descramble_words_dev(d.data_ptr() + off, n, *seed, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            got = d.cpu().numpy()
            want = orc.scramble(words, *seed, 1)
            assert np.array_equal(got[:off], buf[:off]) and np.array_equal(got[off + 9 * n:], buf[off + 9 * n:]), (n, off, seed)   # guards
            if n < 100_000:
                assert np.array_equal(got[off: off + 9 * n], want), (n, off, seed)
            else:
                assert orc.fnv1a64(got[off: off + 9 * n]) == orc.fnv1a64(want), (n, off, seed)
    if n == 1000:                                                             # the host-buffer form
        assert np.array_equal(t3.descramble_words(words.reshape(-1, 9), 2, 1, 0).reshape(-1), orc.scramble(words, 2, 1, 0, 1))


def run_stage_dev(t3, body, hdr, code_k, code_mode, off):
    import torch
    n = len(body)
    total = t3.demap_rsdecode_bands_syms(n, hdr, code_k)
    buf = np.zeros(off + 9 * n + 16, np.uint8); buf[off: off + 9 * n] = np.asarray(body, np.uint8).reshape(-1)
    d_in = _dev(buf)
    d_out = torch.full((off + total + 16,), 0xAB, dtype=torch.uint8, device="cuda")
    d_nv = torch.zeros(1, dtype=torch.int64, device="cuda")
    got_total = t3.demap_rsdecode_bands_dev(d_in.data_ptr() + off, n, hdr, code_k, code_mode, d_out.data_ptr() + off, total, d_nv.data_ptr(),
                                            torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert got_total == total
    assert (out[:off] == 0xAB).all() and (out[off + total:] == 0xAB).all()    # nothing written outside the output
    return int(d_nv.item()), out[off: off + total]


BEACONS = [(0, 0, 0), (1, 0, 1), (2, 8, 1), (3, 9, 1), (83, 200, 1), (83, 4, 0), (2, 0, 1), (3, 8, 1), (83, 0, 1)]


@pytest.mark.gpu
def test_demap_rsdecode_bands_dev(gpu, orc):
    t3 = gpu
    rng = np.random.default_rng(77)
    i = 0
    for n in SIZES:
        for (code_k, code_mode) in CODESETS:
            for bcn in BEACONS:
                i += 1
                hdr = t3.make_cfg(uep=UEPS[i % 3], beacon=bcn)
                corrupt = (0, 1, 3, 5)[i % 4]
                body = stage_body(orc, rng, hdr, code_k, code_mode, n, corrupt)
                ok, want = restate_stage3(orc, body, hdr, code_k, code_mode)
                off = (0, 1, 54)[i % 3]
                nv, got = run_stage_dev(t3, body, hdr, code_k, code_mode, off)
                assert (nv == len(got)) == ok and nv == len(want), (n, code_k, code_mode, bcn, corrupt, nv, len(want))
                assert np.array_equal(got[:nv], want), (n, code_k, code_mode, bcn)
                if i % 7 == 0:                                                # the host-buffer form
                    ok2, syms = t3.demap_rsdecode_bands(body, hdr, code_k, code_mode)
                    assert ok2 == ok and np.array_equal(syms, want)
    # bad codes: T3_E_ARG
    hdr = t3.make_cfg(uep=1)
    with pytest.raises(t3.T3Error):
        t3.demap_rsdecode_bands(np.zeros((52, 9), np.uint8), hdr, [24, 21, 20, 18], (0, 0, 0, 0))
    assert t3.demap_rsdecode_bands_syms(52, hdr, [24, 21, 20, 18]) == 0
    assert t3.demap_rsdecode_bands_syms(52, hdr, [21, 22, 20, 18]) == 9 * 2 * 22         # an unused code is not looked at


@pytest.mark.gpu
def test_demap_rsdecode_bands_one_failure(gpu, orc):
    """Exactly one uncorrectable block, in the middle of band 4: T3_E_RS, the valid prefix = that block's output offset."""
    t3 = gpu
    rng = np.random.default_rng(78)
    n = 26 * 40 + 11
    for code_k, code_mode in CODESETS[:3]:
        hdr = t3.make_cfg(uep=UEPS[0], beacon=(3, 2, 1))
        body = stage_body(orc, rng, hdr, code_k, code_mode, n, 0)
        q = hdr.band_profile[4] % 4; k = code_k[q]
        while True:                                                           # a word the decoder does not take
            junk = rng.integers(0, 27, 26, dtype=np.uint8)
            if not orc.rs_decode_blocks(k, junk, mode=code_mode[q])[2][0]:
                break
        m = 17
        body[26 * m: 26 * m + 26, 4] = junk
        off, total = band_offsets(n, hdr, code_k)
        ok, want = restate_stage3(orc, body, hdr, code_k, code_mode)
        assert not ok and len(want) == off[4] + m * k
        for o in (0, 1, 54):
            nv, got = run_stage_dev(t3, body, hdr, code_k, code_mode, o)
            assert nv == off[4] + m * k and np.array_equal(got[:nv], want)
        ok2, syms = t3.demap_rsdecode_bands(body, hdr, code_k, code_mode)
        assert not ok2 and np.array_equal(syms, want)


@pytest.mark.gpu
def test_demap_rsdecode_bands_8k(gpu, orc):
    """An 8K body (20,766,720 words, RS(26,20) on every band), clean and with <= 3 errors in ~30 % of the blocks, in both arithmetics:
    compared with the restatement by hash."""
    t3 = gpu
    rng = np.random.default_rng(79)
    for code_mode, corrupt in (((0, 0, 0, 0), 0), ((1, 1, 1, 1), 3), ((0, 0, 0, 0), 3)):
        hdr = t3.make_cfg(uep=2)
        body = stage_body(orc, rng, hdr, KS, code_mode, N8K, corrupt)
        ok, want = restate_stage3(orc, body, hdr, KS, code_mode)
        nv, got = run_stage_dev(t3, body, hdr, KS, code_mode, 54 if corrupt else 0)
        assert nv == len(want) and (nv == len(got)) == ok
        assert orc.fnv1a64(got[:nv]) == orc.fnv1a64(want)


def mirror_decode_profile(t3, orc, stream):
    """The mirror's three stages composed as OLD:995-1041 (de-interleave and regroup restated) -> (ok, words, cfg_last_seen)."""
    seen = make_cfg()
    ok, cur, h, fs, bh = t3.read_and_decode_header_from_words(stream, 0, t3.MODE_COMPAT)
    if not ok:
        return False, np.zeros((0, 9), np.uint8), seen
    for f in SEEN_FIELDS:
        setattr(seen, f, getattr(h, f))
    for i in range(9):
        seen.band_profile[i] = h.band_profile[i]
    body = t3.descramble_words(np.asarray(stream, np.uint8).reshape(-1, 9)[cur:], h.seed_a, h.seed_b, h.seed_s0)
    ok, use = t3.demap_rsdecode_bands(body, h, KS, (0, 0, 0, 0))
    if not ok:
        return False, np.zeros((0, 9), np.uint8), seen
    if h.profile == 4 and h.tile_w and h.tile_h:
        use = orc.interleave2d(use, h.tile_w, h.tile_h, 1)
    return True, regroup_words(use), seen


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(STAGE_CFGS))
def test_mirror_stages_compose_to_decode_profile(gpu, orc, name):
    for nbw, corrupt, s in stage_streams(orc, name):
        sa = make_cfg()
        ra, a = orc.decode_profile(s, sa)
        ok, words, seen = mirror_decode_profile(gpu, orc, s)
        assert (ra == 0) == ok and np.array_equal(a, words) and sa.as_dict() == seen.as_dict(), (name, nbw, corrupt)


@pytest.mark.gpu
def test_stage_names_on_device(gpu, orc, tmp_path):
    """stage_names_demo's spelled-out decode_profile_to_raw (the three stage names + deinterleave2D_boustrophedon + trit regroup, as
    OLD:995-1041) equals the drop-in decode_profile_to_raw and the oracle on decoder-consistent streams."""
    exe = build_stage_demo(str(tmp_path))
    paths, want = [], []
    for name in sorted(STAGE_CFGS):
        for nbw, corrupt, s in stage_streams(orc, name):
            if nbw not in (0, 27, 600):
                continue
            p = os.path.join(str(tmp_path), "s%03d.bin" % len(paths))
            np.ascontiguousarray(s, np.uint8).tofile(p)
            sa = make_cfg()
            ra, a = orc.decode_profile(s, sa)
            paths.append(p); want.append((ra == 0, a, sa))
    out = json.loads(subprocess.run([exe, "dev", *paths], check=True, capture_output=True, text=True).stdout)
    assert out["status"] == 0 and len(out["streams"]) == len(want)
    for got, (ok, a, sa) in zip(out["streams"], want):
        assert got["ok_spelled"] == got["ok_dropin"] == int(ok)
        assert got["n_spelled"] == got["n_dropin"] == len(a) and got["h_spelled"] == got["h_dropin"] == ol.fnv_hex(a)
        d = sa.as_dict()
        for s in (got["seen_spelled"], got["seen_dropin"]):
            assert s["band_profile"] == d["band_profile"] and all(s[f] == d[f] for f in SEEN_FIELDS)
