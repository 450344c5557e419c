"""Every device entry point held to its output bounds, to its capacity argument and to the alignment contract of include/t3hip.h.

Buffers are tests/bounds.py's: GUARD bytes of fill around a window of EXACTLY the bytes the plan says the call reads or writes (no slack),
every case once with fill 0xA5 and once with 0x5A in all guards and in the output window.  The expected bytes come from the CPU oracle
(oracle/t3_oracle.c) or numpy, never from another GPU call.  One comparison per pass then catches a store in front of or behind the
window, a byte of the window that is never written (one of the two fills differs from the expected byte), and a result that depends on
bytes outside the input.  Inputs must come back as they were uploaded.  tests/test_bounds_helper.py shows, without a GPU, that the checker
reports each of these mistakes.  (An over-read that only discards what it read cannot be seen this way and is not looked for.)

Sizes: the small unit counts of test_encode_frame_vs_oracle / rs_patterns.SMALL_PX, and per configuration one odd count of at least three
tiles whose last block is zero-padded in every band -- the largest frames of this file.  A tile holds whole blocks of every band, so a
padded last block also means a ragged last tile.
  encoder tile   plan_encode (t3_api_encode.cpp) picks 9 Lq <= 60000 symbols: more than 2 * 60000 regrouped symbols are at least three tiles
  decoder tile   fused 9 * 52 * k symbols, one-launch UEP <= 12000, two-kernel <= 16384 (t3_dec_plan.cpp, pinned by test_dec_plan.py): more than 2 * 16384 symbols"""
import ctypes as C
import functools
import os
import zlib

import numpy as np
import pytest

import bounds
import oracle_lib as ol
import rs_patterns as rp
from test_gpu_fixed_errors import KNOBS, OUTPUTS
from test_gpu_parity import CFGS

pytestmark = pytest.mark.gpu

ENC_TILE_SYMS, DEC_TILE_SYMS = 60000, 16384
SMALL_UNITS = (0, 1, 2, 5, 64, 539, 540, 541, 2161)
CRC_MFMA_BYTES = 64 * 2048                       # plan_crc (t3_api_record.cpp): the matrix-core kernel from this many bytes on


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def t3mod():
    import __graft_entry__ as ge
    return ge.load_package()


def u8(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


def padded_odd_px(plan, enough, start):
    """The first odd pixel count from `start` on that is enough(n_px) and whose last block is zero-padded in every band (the search of
    rs_patterns.frame_sizes for 'padded', started from a tile count instead of the error schedule).  plan(n_raw) -> FIXED layout."""
    n = start | 1
    while True:
        L = plan((n + 1) // 2)
        if enough(n, L) and all(int(L.band_len[b]) % int(L.band_k[b]) for b in range(9)):
            return n
        n += 2


def more_syms_than(min_syms):
    return (lambda n, L: int(L.n_sym) > min_syms), 2 * (3 * min_syms // 26) - 1      # n_sym = ceil(26 n_raw / 3): start just below the mark


def one_launch_framing(kw):
    """One k on all bands, 1-D, no beacon: the framing whose tile count t3hip_frames_plan tells (pixel input, both modes)."""
    return not kw.get("beacon", (0, 0, 0))[2] and kw["profile"] != 4 and (kw["uep"] != "luma" and isinstance(kw["uep"], int))


@functools.lru_cache(maxsize=None)
def enc_three_tiles(name):
    t3 = t3mod(); kw = dict(CFGS[name])
    if kw.get("beacon", (0, 0, 0))[1] >= 9:
        kw.pop("beacon")                                  # (FIXED refuses a beacon slot >= 9; the band lengths are the same without it)
    cfg = t3.make_cfg(mode=1, **kw)
    plan = lambda n_raw: t3.plan(n_raw, cfg)
    if not one_launch_framing(kw):
        return padded_odd_px(plan, *more_syms_than(2 * ENC_TILE_SYMS))
    tiles = lambda n: min(t3.frames_plan(False, n, 2, t3.make_cfg(mode=m, **kw), t3.FRAMES_PIXELS).tiles_per_frame for m in (0, 1))
    lo, hi = 1, 1 << 16
    while lo < hi:
        mid = (lo + hi) // 2
        if tiles(mid) >= 3: hi = mid
        else: lo = mid + 1
    return padded_odd_px(plan, lambda n, L: tiles(n) >= 3, lo)


@functools.lru_cache(maxsize=None)
def dec_three_tiles(name):
    t3 = t3mod(); cfg = t3.make_cfg(mode=1, **rp.CONFIGS[name])
    return padded_odd_px(lambda n_raw: t3.plan(n_raw, cfg), *more_syms_than(2 * DEC_TILE_SYMS))


def rand_rgb(rng, n):
    return rng.integers(0, 256, 3 * n, dtype=np.uint8)


# ---- encoders ------------------------------------------------------------------------------------------------------------------------------
def run_encode(gpu, fn, units_bytes, n_units, cfg, want, label, in_off=0):
    """One encode entry on a guarded input and an output of exactly the planned size, both fills."""
    n_raw_cap = len(want) // 9
    for fill in bounds.FILLS:
        src = bounds.Buf(0, fill, in_off, data=units_bytes, name="%s input" % (label,))
        out = bounds.Buf(9 * n_raw_cap, fill, 0, name="%s coded words" % (label,))
        n = fn(src.ptr, n_units, cfg, out.ptr, n_raw_cap, stream())
        bounds.sync()
        assert n == n_raw_cap, (label, n, n_raw_cap)
        src.result()
        out.expect(want)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", sorted(CFGS))
def test_encoders_write_exactly_their_words(gpu, orc, name, mode):
    """t3hip_encode_frame_dev, t3hip_encode_rgb_dev and t3hip_encode_profile_dev on every configuration of test_gpu_parity.CFGS, COMPAT and
    FIXED: the fused single-k kernel of the three front ends, encode_kernel_uep, the four-code two-launch path, both 2-D placements, the
    beacon in the stores and the beacon pass (slot 9, and forced by T3HIP_BEACON_PASS on the beaconed configurations).  Capacity =
    t3hip_encoded_words, output buffer = 9 * that many bytes."""
    cfg, ocfg = gpu.make_cfg(mode=mode, **CFGS[name]), ol.make_cfg(mode=mode, **CFGS[name])
    rng = np.random.default_rng(zlib.crc32(name.encode()) + 100 + mode)
    big = enc_three_tiles(name)
    if mode == 1 and ocfg.beacon_enabled and ocfg.beacon_band_slot >= 9:     # no FIXED framing (t3hip_plan: T3_E_ARG): refused, nothing written
        n = 541; rgb = rand_rgb(rng, n); px = orc.rgb_to_quant(rgb); raw = rng.integers(0, 27, ((n + 1) // 2, 9), dtype=np.uint8)
        assert orc.encode_frame(px, ocfg, cap=n + 64)[0] != 0
        for fill in bounds.FILLS:
            for fn, data, n_units in ((gpu.encode_frame_dev, u8(px), n), (gpu.encode_rgb_dev, rgb, n), (gpu.encode_profile_dev, u8(raw), (n + 1) // 2)):
                src = bounds.Buf(0, fill, 0, data=data, name="input"); out = bounds.Buf(9 * n, fill, 0, name="output")
                with pytest.raises(gpu.T3Error) as e:
                    fn(src.ptr, n_units, cfg, out.ptr, n, stream())
                bounds.sync()
                assert e.value.code == gpu.E_ARG
                src.untouched(); out.untouched()
        return
    if one_launch_framing(CFGS[name]):                                     # this framing tells its tile count
        p = gpu.frames_plan(False, big, 2, cfg, gpu.FRAMES_PIXELS)
        assert p.one_launch and p.tiles_per_frame >= 3, (name, big, p.tiles_per_frame)
    assert big < 40_000, (name, big)
    for n in SMALL_UNITS + (big,):
        rgb = rand_rgb(rng, n)
        px = orc.rgb_to_quant(rgb)                                           # the pixel and the RGB front end code the same pixels
        rc, want = orc.encode_frame(px, ocfg, cap=n + 64); assert rc == 0
        want = u8(want)
        assert len(want) == 9 * gpu.encoded_words((n + 1) // 2, cfg), (name, n)
        run_encode(gpu, gpu.encode_frame_dev, u8(px), n, cfg, want, (name, mode, n, "pixels"))
        run_encode(gpu, gpu.encode_rgb_dev, rgb, n, cfg, want, (name, mode, n, "rgb"))
    for n_raw in sorted({n // 2 for n in SMALL_UNITS} | {(big + 1) // 2}):
        raw = rng.integers(0, 27, (n_raw, 9), dtype=np.uint8)
        rc, want = orc.encode_profile(raw, ocfg); assert rc == 0
        want = u8(want)
        assert len(want) == 9 * gpu.encoded_words(n_raw, cfg), (name, n_raw)
        run_encode(gpu, gpu.encode_profile_dev, u8(raw), n_raw, cfg, want, (name, mode, n_raw, "raw words"))
    if ocfg.beacon_enabled:                                                  # the separate beacon pass instead of the beacon in the stores
        n = big; rgb = rand_rgb(rng, n); px = orc.rgb_to_quant(rgb)
        rc, want = orc.encode_frame(px, ocfg, cap=n + 64); assert rc == 0
        os.environ["T3HIP_BEACON_PASS"] = "1"
        try:
            run_encode(gpu, gpu.encode_frame_dev, u8(px), n, cfg, u8(want), (name, mode, n, "pixels, beacon pass"))
            run_encode(gpu, gpu.encode_rgb_dev, rgb, n, cfg, u8(want), (name, mode, n, "rgb, beacon pass"))
        finally:
            os.environ.pop("T3HIP_BEACON_PASS", None)


# ---- FIXED decoders ------------------------------------------------------------------------------------------------------------------------
class DecFrame:
    """One FIXED frame of rs_patterns.CONFIGS: the oracle's stream with 0..t symbol errors in every block (t: the frame's weakest band,
    errors applied by the oracle's injector on the host, to the body without its beacon symbols), and what the oracle decodes it to."""

    def __init__(self, orc, name, n_px):
        t3 = t3mod()
        cfg = t3.make_cfg(mode=1, **rp.CONFIGS[name])
        fr = rp.Frame(orc, lambda n_raw: t3.plan(n_raw, cfg), name, n_px, 7)
        L = fr.L
        t = (26 - max(fr.ks)) // 2
        flat = fr.clean.reshape(-1).copy()
        bi = rp.body_index(L, fr.ocfg)
        assert len(bi) == int(L.body_syms)
        body = np.zeros((len(bi) + 8) // 9 * 9, np.uint8); body[: len(bi)] = flat[bi]
        bad = u8(orc.inject_errors(body.reshape(-1, 9), 0, len(bi) // 26, 4242 + n_px, t))
        flat[bi] = bad[: len(bi)]
        assert (flat != fr.clean.reshape(-1)).any() or len(bi) < 3 * 26, "no error placed"
        rc, px = orc.decode_frame(flat.reshape(-1, 9), ol.make_cfg(mode=1))
        assert rc == 0 and np.array_equal(px, fr.padded), (name, n_px)
        self.name, self.n_px, self.n_raw, self.n_in = name, n_px, fr.n_raw, len(flat) // 9
        self.stream = flat
        self.want = {True: u8(px), False: u8(orc.pack_pixels(px))}
        self.rgb = {n: u8(orc.quant_to_rgb(px[:n])) for n in (2 * fr.n_raw, 2 * fr.n_raw - 1)}
        for a in (self.stream, self.want[True], self.want[False]) + tuple(self.rgb.values()):
            a.setflags(write=False)

    def units(self, to_pixels):
        return (2 * self.n_raw, 6) if to_pixels else (self.n_raw, 9)


@functools.lru_cache(maxsize=8)
def dec_frame(name, n_px):
    return DecFrame(ol.oracle(), name, n_px)


def dec_sizes(name):
    return (1, rp.SMALL_PX, dec_three_tiles(name))


def run_decoders(gpu, fr, outputs, label, in_off=0, out_off=0, rgb=True, entries=("async", "sync", "body")):
    """The frame through t3hip_decode_frame_async, t3hip_decode_profile_dev, t3hip_decode_body_dev (pixels / raw words) and
    t3hip_decode_rgb_async (both pixel counts of the frame): capacity exactly the plan's, output and verdict words guarded."""
    cfg = gpu.make_cfg(mode=1, **rp.CONFIGS[fr.name])
    s = stream()
    for fill in bounds.FILLS:
        src = bounds.Buf(0, fill, in_off, data=fr.stream, name="%s coded input" % (label,))
        for to_pixels in outputs:
            n, sz = fr.units(to_pixels)
            for entry in entries:
                what = "%s %s %s" % (label, entry, "pixels" if to_pixels else "raw words")
                out = bounds.Buf(n * sz, fill, out_off, name=what + " output")
                ver = bounds.Buf(8, fill, 0, name=what + " verdict words")
                fail = bounds.Buf(0, fill, 0, data=np.zeros(4, np.uint8), name=what + " failure counter")
                if entry == "async":
                    got = gpu.decode_frame_async(src.ptr, fr.n_in, cfg, fr.n_raw, out.ptr, n, ver.ptr, to_pixels, s)
                elif entry == "sync":
                    rc, got = gpu.decode_profile_dev(src.ptr, fr.n_in, gpu.DecoderContext(mode=1).cfg_last_seen, out.ptr, n, to_pixels, s)
                    assert rc == 0, (what, rc)
                else:
                    got = gpu.decode_body_dev(src.ptr, fr.n_in, cfg, fr.n_raw, out.ptr, n, fail.ptr, to_pixels, s)
                bounds.sync()
                assert got == n, (what, got, n)
                out.expect(fr.want[to_pixels])
                fail.result()                                                 # still zero: no block failed, nothing else written
                if entry == "async":
                    ver.expect(np.zeros(8, np.uint8))                         # [0, 0]: the eight bytes the entry may write
                else:
                    ver.untouched()
        if rgb:
            for n_px, want in fr.rgb.items():
                what = "%s rgb %d px" % (label, n_px)
                out = bounds.Buf(3 * n_px, fill, out_off, name=what + " output")
                ver = bounds.Buf(8, fill, 0, name=what + " verdict words")
                gpu.decode_rgb_async(src.ptr, fr.n_in, cfg, n_px, out.ptr, ver.ptr, s)
                bounds.sync()
                out.expect(want)
                ver.expect(np.zeros(8, np.uint8))
        src.result()


@pytest.mark.parametrize("name", sorted(rp.CONFIGS))
def test_fixed_decoders_write_exactly_their_units(gpu, orc, name):
    """Every framing of rs_patterns.CONFIGS (fused kernel with and without a beacon in its loads, one-launch UEP / 2-D kernel, two-kernel
    decoder; raw-word output where test_gpu_fixed_errors.OUTPUTS lists it) at 1 pixel, SMALL_PX and three padded tiles, with errors in
    every block so that the correctors write."""
    for n_px in dec_sizes(name):
        fr = dec_frame(name, n_px)
        if n_px > rp.SMALL_PX and name in rp.ONE_K:                           # the tile-range plan tells this framing's tile count
            cfg = gpu.make_cfg(mode=1, **rp.CONFIGS[name])
            assert gpu.window_plan(fr.n_raw, cfg, 2 * fr.n_raw, 1, 0, 0, 2 * fr.n_raw, 1).n_tiles >= 3
        assert n_px < 12_000
        run_decoders(gpu, fr, OUTPUTS[name], (name, n_px))


@pytest.mark.parametrize("knob,name", KNOBS)
def test_fixed_decoders_forced_paths_write_exactly_their_units(gpu, orc, knob, name):
    """The generic gather decoder and the two-kernel decoder forced by their knobs, on the same frames: the bytes are those of the planned
    decoder above (both equal the oracle's), so a capacity that is exactly right did not send that run to the generic kernels unnoticed."""
    os.environ[knob] = "1"
    try:
        for n_px in dec_sizes(name):
            run_decoders(gpu, dec_frame(name, n_px), OUTPUTS[name], (knob, name, n_px))
    finally:
        os.environ.pop(knob, None)


@pytest.mark.parametrize("name", ["p3_uniform20", "p5_tile64_luma", "p1_beacon3_slot8"])
def test_compat_generic_decoder_writes_exactly_its_units(gpu, orc, name):
    """COMPAT streams go through the generic kernels: decoder-consistent streams of 27 and 600 body words, words and pixels out."""
    from test_oracle_vs_ref import decoder_consistent_stream
    rng = np.random.default_rng(zlib.crc32(name.encode()) + 19)
    ocfg = ol.make_cfg(**CFGS[name])
    s = stream()
    for nbw in (27, 600):
        words = decoder_consistent_stream(orc, rng, ocfg, nbw, 0)
        rc, want = orc.decode_profile(words, ol.make_cfg())
        assert rc == 0 and len(want) > 0, (name, nbw)
        expect = {False: u8(want), True: u8(orc.unpack_words(want))}
        for fill in bounds.FILLS:
            src = bounds.Buf(0, fill, 0, data=u8(words), name="%s %d coded input" % (name, nbw))
            for to_pixels in (False, True):
                n = 2 * len(want) if to_pixels else len(want)
                out = bounds.Buf(len(expect[to_pixels]), fill, 0, name="%s %d %s" % (name, nbw, "pixels" if to_pixels else "words"))
                rcd, got = gpu.decode_profile_dev(src.ptr, len(words), gpu.DecoderContext().cfg_last_seen, out.ptr, n, to_pixels, s)
                bounds.sync()
                assert rcd == 0 and got == n, (name, nbw, to_pixels, rcd, got)
                out.expect(expect[to_pixels])
            src.result()


# ---- alignment (include/t3hip.h, conventions) --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["k20", "luma"])
def test_decode_misaligned_pixel_destination_goes_generic(gpu, orc, name):
    """A pixel destination that is not 16-byte aligned is accepted: the generic kernels take the frame.  Offsets 2, 6 and 8 behind a
    16-byte boundary, output and guards right, through the three pixel entries."""
    for n_px in (rp.SMALL_PX, dec_three_tiles(name)):
        for off in (2, 6, 8):
            run_decoders(gpu, dec_frame(name, n_px), (True,), (name, n_px, "destination + %d" % off), out_off=off, rgb=(off == 2))


@pytest.mark.parametrize("name", ["k20", "luma", "four_codes"])
def test_decode_misaligned_word_and_rgb_destination(gpu, orc, name):
    """Raw words go out at any address (the fused word kernel and the two-kernel decoder store bytes up to the first 16-byte boundary),
    RGB too (the pixel scratch and the bridge kernel): offsets 1, 2 and 8."""
    for n_px in (rp.SMALL_PX, dec_three_tiles(name)):
        for off in (1, 2, 8):
            run_decoders(gpu, dec_frame(name, n_px), (False,), (name, n_px, "destination + %d" % off), out_off=off, rgb=True)


@pytest.mark.parametrize("name", ["k20", "k20_beacon83", "luma", "four_codes", "2d_64x64_k20"])
def test_decode_misaligned_input_is_accepted(gpu, orc, name):
    """The decode entries read a coded stream at any even address (16-byte alignment is the fast path, not a condition): offsets 2, 6
    and 8, through every FIXED decoder, same bytes out, nothing outside the input taken into the result."""
    for n_px in (rp.SMALL_PX, dec_three_tiles(name)):
        for off in (2, 6, 8):
            run_decoders(gpu, dec_frame(name, n_px), OUTPUTS[name], (name, n_px, "input + %d" % off), in_off=off, rgb=(off == 8), entries=("async", "sync"))


@pytest.mark.parametrize("name", ["k20", "luma"])
def test_decode_odd_addresses_are_refused(gpu, orc, name):
    """A coded stream at an odd address (offsets 1 and 7), and a pixel destination at one, are T3_E_ARG from every profile decode entry:
    nothing launched, output and verdict words untouched."""
    fr = dec_frame(name, rp.SMALL_PX)
    cfg = gpu.make_cfg(mode=1, **rp.CONFIGS[name]); s = stream()
    for fill in bounds.FILLS:
        for in_off, out_off, outputs in ((1, 0, (True, False)), (7, 0, (True, False)), (0, 1, (True,))):
            src = bounds.Buf(0, fill, in_off, data=fr.stream, name="coded input + %d" % in_off)
            for to_pixels in outputs:
                n, sz = fr.units(to_pixels)
                out = bounds.Buf(n * sz, fill, out_off, name="output + %d" % out_off)
                ver = bounds.Buf(8, fill, 0, name="verdict words")
                calls = [lambda: gpu.decode_frame_async(src.ptr, fr.n_in, cfg, fr.n_raw, out.ptr, n, ver.ptr, to_pixels, s),
                         lambda: gpu.decode_profile_dev(src.ptr, fr.n_in, gpu.DecoderContext(mode=1).cfg_last_seen, out.ptr, n, to_pixels, s),
                         lambda: gpu.decode_body_dev(src.ptr, fr.n_in, cfg, fr.n_raw, out.ptr, n, ver.ptr, to_pixels, s)]
                if in_off:
                    calls.append(lambda: gpu.decode_rgb_async(src.ptr, fr.n_in, cfg, 2 * fr.n_raw, out.ptr, ver.ptr, s))
                for call in calls:
                    with pytest.raises(gpu.T3Error) as e:
                        call()
                    bounds.sync()
                    assert e.value.code == gpu.E_ARG, (name, in_off, out_off, to_pixels, e.value.code)
                    src.untouched(); out.untouched(); ver.untouched()


def test_encode_misaligned_buffers_are_refused(gpu, orc):
    """Profile encode entries: a device buffer 8 bytes off a 16-byte boundary, in front of it or behind, is T3_E_ARG and nothing is written.
    (RGB input is the exception t3hip.h names: any alignment, the bridge kernel takes it; its coded output must be aligned all the same.)"""
    n = 541
    cfg, ocfg = gpu.make_cfg(profile=2, uep=2), ol.make_cfg(profile=2, uep=2)
    rng = np.random.default_rng(5)
    rgb = rand_rgb(rng, n); px = orc.rgb_to_quant(rgb)
    raw = rng.integers(0, 27, ((n + 1) // 2, 9), dtype=np.uint8)
    rc, want = orc.encode_frame(px, ocfg, cap=n + 64); assert rc == 0
    cap = len(want)
    cases = [("pixels", gpu.encode_frame_dev, u8(px), n), ("raw words", gpu.encode_profile_dev, u8(raw), (n + 1) // 2), ("rgb", gpu.encode_rgb_dev, rgb, n)]
    for fill in bounds.FILLS:
        for label, fn, data, n_units in cases:
            for d_in, d_out in ((8, 0), (-8, 0), (0, 8), (0, -8)):
                if label == "rgb" and d_in:
                    continue
                src = bounds.Buf(0, fill, 0, data=data, name=label + " input")
                out = bounds.Buf(9 * cap + 8, fill, 0, name=label + " output")
                with pytest.raises(gpu.T3Error) as e:
                    fn(src.ptr + d_in, n_units, cfg, out.ptr + d_out, cap, stream())
                bounds.sync()
                assert e.value.code == gpu.E_ARG, (label, d_in, d_out, e.value.code)
                src.untouched(); out.untouched()
        for off in (1, 8):                                                    # RGB input off the boundary: accepted, same stream
            src = bounds.Buf(0, fill, off, data=rgb, name="rgb input + %d" % off)
            out = bounds.Buf(9 * cap, fill, 0, name="rgb coded words")
            assert gpu.encode_rgb_dev(src.ptr, n, cfg, out.ptr, cap, stream()) == cap
            bounds.sync()
            src.result(); out.expect(u8(want))


# ---- the other device entries --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("off", [0, 2, 6, 8])
def test_pack_unpack_dev_bounds(gpu, orc, off):
    rng = np.random.default_rng(60 + off)
    s = stream()
    for n in (1, 2, 3, 7, 1001):
        px = rp.rand_pixels(rng, n)
        words = rng.integers(0, 27, (n, 9), dtype=np.uint8)
        want_w, want_px = u8(orc.pack_pixels(px)), u8(orc.unpack_words(words))
        for fill in bounds.FILLS:
            src = bounds.Buf(0, fill, off, data=u8(px), name="pack %d px input" % n)
            out = bounds.Buf(9 * ((n + 1) // 2), fill, off, name="pack %d px -> words" % n)
            gpu.pack_pixels_dev(src.ptr, n, out.ptr, s)
            src2 = bounds.Buf(0, fill, off, data=u8(words), name="unpack %d words input" % n)
            out2 = bounds.Buf(12 * n, fill, off, name="unpack %d words -> pixels" % n)
            gpu.unpack_words_dev(src2.ptr, n, out2.ptr, s)
            bounds.sync()
            src.result(); out.expect(want_w); src2.result(); out2.expect(want_px)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("k", [24, 22, 20, 18])
def test_rs_blocks_dev_bounds(gpu, orc, k, mode):
    """Block-level RS around the sets of 32 the matrix-core kernels work in.  Decode: d_code26 is corrected in place (the whole 26 n bytes
    may change, and must equal the oracle's), d_data_k of a block that does not decode keeps what it held -- the fill -- as t3hip.h says."""
    rng = np.random.default_rng(1000 * k + mode)
    s = stream(); t = (26 - k) // 2
    for n in (1, 31, 32, 33, 63, 64, 65, 1000):
        data = rng.integers(0, 27, (n, k), dtype=np.uint8)
        code = orc.rs_encode_blocks(k, data, mode)
        rx = orc.rs_encode_blocks(k, data, 1)
        for i, row in enumerate(rx):                                          # 0 .. t + 1 errors: some blocks do not decode
            e = i % (t + 2); pos = rng.choice(26, e, replace=False)
            row[pos] = (row[pos] + rng.integers(1, 27, e)) % 27
        oc, odk, ook = orc.rs_decode_blocks(k, rx, mode)
        for fill in bounds.FILLS:
            src = bounds.Buf(0, fill, 0, data=u8(data), name="rs encode k=%d n=%d data" % (k, n))
            out = bounds.Buf(26 * n, fill, 0, name="rs encode k=%d n=%d code" % (k, n))
            gpu.rs_encode_blocks_dev(k, mode, src.ptr, n, out.ptr, s)
            inout = bounds.Buf(0, fill, 0, data=u8(rx), name="rs decode k=%d n=%d code (in place)" % (k, n), may_change=[(0, 26 * n)])
            dk = bounds.Buf(k * n, fill, 0, name="rs decode k=%d n=%d data" % (k, n))
            ok = bounds.Buf(n, fill, 0, name="rs decode k=%d n=%d ok" % (k, n))
            gpu.rs_decode_blocks_dev(k, mode, inout.ptr, n, dk.ptr, ok.ptr, s)
            bounds.sync()
            src.result(); out.expect(code)
            ok.expect(ook)
            bounds.check_equal(inout.result(), u8(oc), fill, inout.name)
            dk.expect(np.where(ook[:, None] == 1, odk, np.uint8(fill)).astype(np.uint8))


@pytest.mark.parametrize("offs", [(0, 0), (1, 2), (3, 6), (6, 8), (8, 2), (15, 14)])
def test_rgb_bridge_dev_bounds(gpu, orc, offs):
    rng = np.random.default_rng(offs[0])
    s = stream()
    for n in (1, 3, 4, 5, 4097):
        rgb = rand_rgb(rng, n); px = rp.rand_pixels(rng, n)
        want_px, want_rgb = u8(orc.rgb_to_quant(rgb)), u8(orc.quant_to_rgb(px))
        for fill in bounds.FILLS:
            src = bounds.Buf(0, fill, offs[0], data=rgb, name="rgb_to_quant %d input" % n)
            out = bounds.Buf(6 * n, fill, offs[1], name="rgb_to_quant %d pixels" % n)
            gpu.rgb_to_quant_dev(src.ptr, n, out.ptr, s)
            src2 = bounds.Buf(0, fill, offs[1], data=u8(px), name="quant_to_rgb %d input" % n)
            out2 = bounds.Buf(3 * n, fill, offs[0], name="quant_to_rgb %d rgb" % n)
            gpu.quant_to_rgb_dev(src2.ptr, n, out2.ptr, s)
            bounds.sync()
            src.result(); out.expect(want_px); src2.result(); out2.expect(want_rgb)


@pytest.mark.parametrize("tile", [(16, 3), (48, 5), (516, 7)])
def test_interleave2d_dev_bounds(gpu, orc, tile):
    """Three tile geometries of test_2d_in_place_flows on a symbol count that is no multiple of the tile (nor of its row); the entry
    writes d_out and leaves d_in alone (t3hip.h: d_out != d_in)."""
    w, h = tile
    rng = np.random.default_rng(w)
    s = stream()
    for n in (3 * w * h + w + 5, w * h - 3, 7):
        syms = rng.integers(0, 27, n, dtype=np.uint8)
        want = orc.interleave2d(syms, w, h)
        for fill in bounds.FILLS:
            for off in (0, 6):
                src = bounds.Buf(0, fill, off, data=syms, name="interleave %s n=%d input" % (tile, n))
                out = bounds.Buf(n, fill, off, name="interleave %s n=%d output" % (tile, n))
                gpu.interleave2d_dev(src.ptr, n, w, h, out.ptr, s)
                bounds.sync()
                src.result(); out.expect(want)


def test_inject_errors_dev_bounds(gpu, orc):
    """Only bytes of [first_sym, first_sym + 26 n_blocks) change, at most max_err per block, and the result is the oracle's."""
    rng = np.random.default_rng(8)
    s = stream()
    for first, nb, max_err, n_words in ((52, 390, 3, 1200), (90, 1, 4, 14), (0, 33, 1, 96), (7, 64, 0, 200)):
        w = rng.integers(0, 27, (n_words, 9), dtype=np.uint8)
        assert first + 26 * nb <= 9 * n_words
        want = u8(orc.inject_errors(w, first, nb, 99, max_err))
        changed = (want != u8(w))[first: first + 26 * nb].reshape(nb, 26).sum(axis=1)
        assert changed.max() <= max_err and (max_err == 0 or changed.any())
        for fill in bounds.FILLS:
            buf = bounds.Buf(0, fill, 0, data=u8(w), name="inject %d blocks at %d" % (nb, first), may_change=[(first, first + 26 * nb)])
            gpu.inject_errors_dev(buf.ptr, first, nb, 99, max_err, s)
            bounds.sync()
            got = buf.result()                                                # guards, and every byte outside the range as uploaded
            bounds.check_equal(got, want, fill, buf.name)


@pytest.mark.parametrize("n_words", [1000, CRC_MFMA_BYTES // 9 + 37])
def test_crc_and_frame_record_bounds(gpu, orc, n_words):
    """t3hip_crc32_dev and t3hip_frame_record_dev on a payload below and one above the matrix-core threshold: the 96-byte record and the
    scratch are the only bytes written, the payload is not."""
    assert (9 * n_words >= CRC_MFMA_BYTES) == (n_words > 1000)
    rng = np.random.default_rng(n_words)
    w = rng.integers(0, 27, (n_words, 9), dtype=np.uint8)
    cfg = gpu.make_cfg(profile=2, uep=2, mode=1)
    rec = gpu.FrameRecord(); rec.frame_idx, rec.n_words, rec.byte_offset, rec.crc32, rec.sym_sum = 11, n_words, 0, orc.crc32(w), orc.sym_sum(w)
    for i in range(54):
        rec.header_syms[i] = int(u8(w)[i])
    rec.profile, rec.mode = 2, 1
    want = np.frombuffer(bytes(rec), np.uint8)
    assert len(want) == 96
    for fill in bounds.FILLS:
        src = bounds.Buf(0, fill, 0, data=u8(w), name="crc payload")
        assert gpu.crc32_dev(src.ptr, 9 * n_words, stream()) == orc.crc32(w)         # synchronous
        src.result()
        for nscr in (64, gpu.frame_record_scratch_bytes(n_words)):
            out = bounds.Buf(96, fill, 0, name="frame record")
            scr = bounds.Buf(nscr, fill, 0, name="record scratch of %d bytes" % nscr)
            gpu.frame_record_dev(src.ptr, n_words, 11, cfg, out.ptr, scr.ptr, nscr, stream())
            bounds.sync()
            out.expect(want); scr.result(); src.result()


# ---- capacity ------------------------------------------------------------------------------------------------------------------------------
def refused(gpu, call, needed, bufs, label):
    """`call` raises T3Error(E_CAPACITY) with the needed size, and after a synchronise no byte of bufs has changed."""
    with pytest.raises(gpu.T3Error) as e:
        call()
    bounds.sync()
    assert e.value.code == gpu.E_CAPACITY, (label, e.value.code)
    assert e.value.needed == needed, (label, e.value.needed, needed)
    for b in bufs:
        b.untouched()


def refused_host(gpu, fill, nbytes, fn, needed, label):
    """A host-buffer entry on a numpy output with guards: fn(output pointer, size pointer) is T3_E_CAPACITY, the size pointer holds the
    size needed, not a byte of the allocation is written."""
    img = bounds.host_image(nbytes, fill); n_out = C.c_uint64(12345)
    rc = fn(C.c_void_p(img.ctypes.data + bounds.window_start(0)), C.byref(n_out))
    assert rc == gpu.E_CAPACITY and n_out.value == needed, (label, rc, n_out.value, needed)
    bounds.check_untouched(img, fill, label)


def test_capacity_one_unit_short_device_encoders(gpu, orc):
    """T3_E_CAPACITY from the encode entries (t3hip_encode_image_dev included): refused before anything is launched on the output,
    *n_out = the words needed."""
    n = 2161
    cfg = gpu.make_cfg(profile=2, uep=2, mode=1)
    rng = np.random.default_rng(12)
    rgb = rand_rgb(rng, n); px = orc.rgb_to_quant(rgb); raw = rng.integers(0, 27, ((n + 1) // 2, 9), dtype=np.uint8)
    need = gpu.encoded_words((n + 1) // 2, cfg)
    fw, fh = gpu.image_geometry(15, 0)[:2]
    need_img = gpu.encoded_words((fw * fh + 1) // 2, cfg)
    img = rand_rgb(rng, 8 * 8)
    for fill in bounds.FILLS:
        for label, fn, data, n_units in (("pixels", gpu.encode_frame_dev, u8(px), n), ("raw words", gpu.encode_profile_dev, u8(raw), (n + 1) // 2), ("rgb", gpu.encode_rgb_dev, rgb, n)):
            src = bounds.Buf(0, fill, 0, data=data, name=label + " input")
            out = bounds.Buf(9 * (need - 1), fill, 0, name=label + " output, one word short")
            refused(gpu, lambda: fn(src.ptr, n_units, cfg, out.ptr, need - 1, stream()), need, (src, out), label)
        src = bounds.Buf(0, fill, 0, data=img, name="image input")
        out = bounds.Buf(4096, fill, 0, name="image output")                  # (the refusal comes before the buffer's size matters)
        refused(gpu, lambda: gpu.encode_image_dev(src.ptr, 8, 8, 15, 0, cfg, out.ptr, need_img - 1, stream()), need_img, (src, out), "image")


@pytest.mark.parametrize("to_pixels", [True, False])
def test_capacity_one_unit_short_device_decoders(gpu, orc, to_pixels):
    """decode_frame_async, decode_profile_dev (header-parsed and RAW mode) and decode_body_dev with room for one unit less than the frame
    has: T3_E_CAPACITY with *n_out = the units needed; output, verdict words and failure counter untouched -- in particular the frame is
    not handed to another decoder instead.  The same frame with the capacity exactly right decodes (test_fixed_decoders_... above)."""
    for name in ("k20", "luma"):
        fr = dec_frame(name, rp.SMALL_PX)
        cfg = gpu.make_cfg(mode=1, **rp.CONFIGS[name])
        n, sz = fr.units(to_pixels); s = stream()
        for fill in bounds.FILLS:
            src = bounds.Buf(0, fill, 0, data=fr.stream, name="coded input")
            out = bounds.Buf((n - 1) * sz, fill, 0, name="output, one unit short")
            ver = bounds.Buf(8, fill, 0, name="verdict words")
            refused(gpu, lambda: gpu.decode_frame_async(src.ptr, fr.n_in, cfg, fr.n_raw, out.ptr, n - 1, ver.ptr, to_pixels, s), n, (src, out, ver), (name, "async"))
            refused(gpu, lambda: gpu.decode_body_dev(src.ptr, fr.n_in, cfg, fr.n_raw, out.ptr, n - 1, ver.ptr, to_pixels, s), n, (src, out, ver), (name, "body"))
            refused(gpu, lambda: gpu.decode_profile_dev(src.ptr, fr.n_in, gpu.DecoderContext(mode=1).cfg_last_seen, out.ptr, n - 1, to_pixels, s), n, (src, out), (name, "sync"))
            seen = gpu.DecoderContext(mode=1).cfg_last_seen; seen.profile = gpu.ProfileID.RAW_MODE
            raw_units = 2 * fr.n_in if to_pixels else fr.n_in
            refused(gpu, lambda: gpu.decode_profile_dev(src.ptr, fr.n_in, seen, out.ptr, raw_units - 1, to_pixels, s), raw_units, (src, out), (name, "sync RAW"))


def test_capacity_one_unit_short_stage_and_subword_entries(gpu, orc):
    """t3hip_demap_rsdecode_bands_dev / _bands, t3hip_subword_build(_dev), t3hip_base243_pack(_dev), t3hip_base243_unpack."""
    rng = np.random.default_rng(3)
    s = stream()
    hdr = gpu.make_cfg(profile=1, uep="luma"); ks, ms = (24, 22, 20, 18), (1, 1, 1, 1)
    n_words = 52
    body = rng.integers(0, 27, (n_words, 9), dtype=np.uint8)
    need = gpu.demap_rsdecode_bands_syms(n_words, hdr, ks)
    assert need == 2 * (3 * 20 + 6 * 22)
    trits = rng.integers(0, 3, 24 * 10 + 5, dtype=np.uint8)
    packed = orc.ut_to_base243(trits)
    L = gpu.lib()
    for fill in bounds.FILLS:
        src = bounds.Buf(0, fill, 0, data=u8(body), name="stage 3 body")
        out = bounds.Buf(need - 1, fill, 0, name="stage 3 symbols, one short")
        nv = bounds.Buf(8, fill, 0, name="stage 3 valid prefix")
        refused(gpu, lambda: gpu.demap_rsdecode_bands_dev(src.ptr, n_words, hdr, ks, ms, out.ptr, need - 1, nv.ptr, s), need, (src, out, nv), "demap_rsdecode_bands_dev")
        tsrc = bounds.Buf(0, fill, 0, data=trits, name="trits")
        wout = bounds.Buf(9 * 10, fill, 0, name="subword words, one short")
        refused(gpu, lambda: gpu.subword_build_dev(tsrc.ptr, len(trits), 24, 0, wout.ptr, 10, s), 11, (tsrc, wout), "subword_build_dev")
        bout = bounds.Buf(len(packed) - 1, fill, 0, name="base243 bytes, one short")
        refused(gpu, lambda: gpu.base243_pack_dev(tsrc.ptr, len(trits), bout.ptr, len(packed) - 1, s), len(packed), (tsrc, bout), "base243_pack_dev")
        host = functools.partial(refused_host, gpu, fill)
        kk, mm = (C.c_uint8 * 4)(*ks), (C.c_uint8 * 4)(*ms)
        host(need - 1, lambda p, n: L.t3hip_demap_rsdecode_bands(body.ctypes.data_as(C.c_void_p), C.c_uint64(n_words), C.byref(hdr), kk, mm, p, C.c_uint64(need - 1), n), need, "demap_rsdecode_bands")
        host(9 * 10, lambda p, n: L.t3hip_subword_build(trits.ctypes.data_as(C.c_void_p), C.c_uint64(len(trits)), C.c_int(24), C.c_uint8(0), p, C.c_uint64(10), n), 11, "subword_build")
        host(len(packed) - 1, lambda p, n: L.t3hip_base243_pack(trits.ctypes.data_as(C.c_void_p), C.c_uint64(len(trits)), p, C.c_uint64(len(packed) - 1), n), len(packed), "base243_pack")
        host(len(trits) - 1, lambda p, n: L.t3hip_base243_unpack(packed.ctypes.data_as(C.c_void_p), C.c_uint64(len(packed)), p, C.c_uint64(len(trits) - 1), n), len(trits), "base243_unpack")


def test_capacity_one_unit_short_host_entries(gpu, orc):
    """t3hip_encode_profile, t3hip_encode_frame, t3hip_decode_profile, t3hip_decode_frame and t3hip_decode_frames on host buffers: a numpy
    output with guards, one unit short -> T3_E_CAPACITY, *n_out = the size needed, not a byte of the output written."""
    L = gpu.lib()
    n = 2161
    rng = np.random.default_rng(14)
    px = rp.rand_pixels(rng, n); raw = rng.integers(0, 27, ((n + 1) // 2, 9), dtype=np.uint8)
    cfg = gpu.make_cfg(profile=2, uep=2, mode=1)
    need = gpu.encoded_words((n + 1) // 2, cfg)
    fr = dec_frame("k20", rp.SMALL_PX)
    words = np.ascontiguousarray(fr.stream)
    for fill in bounds.FILLS:
        host = functools.partial(refused_host, gpu, fill)
        host(9 * (need - 1), lambda p, no: L.t3hip_encode_profile(raw.ctypes.data_as(C.c_void_p), C.c_uint64(len(raw)), C.byref(cfg), p, C.c_uint64(need - 1), no), need, "encode_profile")
        host(9 * (need - 1), lambda p, no: L.t3hip_encode_frame(px.ctypes.data_as(C.c_void_p), C.c_uint64(n), C.byref(cfg), p, C.c_uint64(need - 1), no), need, "encode_frame")
        for to_pixels, fn in ((False, L.t3hip_decode_profile), (True, L.t3hip_decode_frame)):
            units, sz = fr.units(to_pixels)
            seen = gpu.DecoderContext(mode=1).cfg_last_seen
            host(sz * (units - 1), lambda p, no: fn(words.ctypes.data_as(C.c_void_p), C.c_uint64(fr.n_in), C.byref(seen), p, C.c_uint64(units - 1), no), units, fn.__name__)
        # a batch of two such frames, pixels out
        units = 2 * fr.n_raw
        in_stride, out_stride = (9 * fr.n_in + 15) & ~15, (6 * (units - 1) + 15) & ~15
        batch = np.zeros((2, in_stride), np.uint8); batch[:, : 9 * fr.n_in] = words
        seen = gpu.DecoderContext(mode=1).cfg_last_seen; rcs = (C.c_int * 2)()
        host(2 * out_stride, lambda p, no: L.t3hip_decode_frames(batch.ctypes.data_as(C.c_void_p), C.c_uint64(fr.n_in), C.c_uint64(in_stride), C.c_uint32(2), p, C.c_uint64(out_stride),
                                                                 C.c_uint64(units - 1), C.c_int(1), C.byref(seen), no, rcs), units, "decode_frames")
