"""Every encoder and every FIXED decoder at every place a frame can end within its tile.

The sizes are the lattice of tests/frame_ends.py (every word count within two words of a tile boundary any kernel can have, up to 40000
symbols, and every count up to 130); tests/test_frame_ends_lattice.py proves on the CPU that both sides of every tile step are among them.
A frame of many tiles meets one frame end; here every frame is a frame end: the zero-padded last symbol, each band's padded (FIXED) or
dropped (COMPAT) last block, bands that run out of blocks before others, tiles that hold no block for some waves, the pad pixel of an odd
frame, the rest of the last output word, the beacon's tail bytes, the prefetch behind the frame's end.

The yardstick is the CPU oracle's stream of each frame (frame_ends.Sweep), computed once per configuration and mode.  Buffers are
tests/bounds.py's: windows of exactly the bytes the call may read or write between guards, every case with both fills, so that a result
that depends on bytes behind the input's end, or a byte of the last word that is never written, cannot pass.

Decoders: the oracle's FIXED stream with t errors in block 0 and in every band's last block, the padded data position included
(rs_patterns.schedule), must come back as the frame itself -- no oracle decode is needed for that."""
import functools
import os

import numpy as np
import pytest

import bounds
import frame_ends as fe
import oracle_lib as ol
import rs_patterns as rp
from test_gpu_bounds import run_encode, stream, u8
from test_gpu_fixed_errors import KNOBS, OUTPUTS
from test_gpu_frames import decode_batch, encode_batch
from test_gpu_window import crop_np

pytestmark = pytest.mark.gpu

ENC_FRAMINGS = dict(rp.CONFIGS, **{"2d_5000x3_k20": dict(profile=4, uep=2, tile=(5000, 3)),      # the run flow of the 2-D placement
                                   "2d_1x9_k20": dict(profile=4, uep=2, tile=(1, 9))})             # identity rows
FRONT_ENDS = ("pixels", "rgb", "words")
STRIDE_EXTRA = 4112
FAR_EVERY = 10                                    # every 10th frame also runs clean and with one far row
WINDOW_FW, WINDOW_TAIL = 64, 200


def entry(gpu, front_end):
    return {"pixels": gpu.encode_frame_dev, "rgb": gpu.encode_rgb_dev, "words": gpu.encode_profile_dev}[front_end]


# ---- encoders ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,mode,front_end", [(n, m, f) for n in ENC_FRAMINGS for m in (0, 1) for f in FRONT_ENDS])
def test_encoders_at_every_frame_end(gpu, orc, name, mode, front_end):
    """t3hip_encode_frame_dev / _rgb_dev / _profile_dev on every lattice frame: the word count, every byte of the stream, the guards and
    the input.  RGB input sits at every offset 0 .. 15 behind a 16-byte boundary in turn (it may); the other bases are aligned."""
    kw = ENC_FRAMINGS[name]
    cfg = gpu.make_cfg(mode=mode, **kw)
    sw = fe.sweep(name, kw, mode)
    for i, W in enumerate(sw.Ws):
        data, n_units, want = sw.case(front_end, i)
        assert len(want) == 9 * gpu.encoded_words(W, cfg), (name, mode, W)
        run_encode(gpu, entry(gpu, front_end), data, n_units, cfg, want, (name, mode, front_end, W, n_units), in_off=i % 16 if front_end == "rgb" else 0)


def has_body(W, k, mode):
    """FIXED: any frame of at least a word; COMPAT: band 0, the longest, holds a whole block."""
    return W >= 1 and (mode == 1 or -(-fe.n_sym(W) // 9) >= k)


@pytest.mark.parametrize("name,mode,front_end", [(n, m, f) for n in rp.ONE_K for m in (0, 1) for f in ("pixels", "rgb")])
def test_batched_encode_at_every_frame_end(gpu, orc, name, mode, front_end):
    """t3hip_encode_frames_dev, three different frames per lattice size, at the plan's minimal strides and at those + 4112 with the gaps
    filled: in the tile space frame f's last tile is followed by frame f + 1's first.  Every frame is the oracle's stream of its own
    content; gaps and guards are untouched (test_gpu_frames.encode_batch looks at every byte of them)."""
    kw = rp.CONFIGS[name]; k = fe.band_codes(kw)[0]
    cfg = gpu.make_cfg(mode=mode, **kw)
    sws = [fe.sweep(name, kw, mode, salt) for salt in (0, 1, 2)]
    fmt = gpu.FRAMES_PIXELS if front_end == "pixels" else gpu.FRAMES_RGB
    for i, W in enumerate(sws[0].Ws):
        cases = [s.case(front_end, i) for s in sws]
        n_units = cases[0][1]
        for extra in (0, STRIDE_EXTRA):
            p, got = encode_batch(gpu, [c[0] for c in cases], n_units, fmt, cfg, extra)
            assert p.one_launch == (1 if has_body(W, k, mode) else 0), (name, mode, front_end, W)
            for f, c in enumerate(cases):
                assert np.array_equal(got[f], c[2]), (name, mode, front_end, W, extra, "frame %d differs from the oracle" % f)


# ---- FIXED decoders ------------------------------------------------------------------------------------------------------------------------
class Corrupted:
    """The FIXED sweep of one configuration (in-range frames, salt as in frame_ends.Sweep) with the <= t schedule applied to every frame."""

    def __init__(self, t3, name, salt):
        kw = rp.CONFIGS[name]
        self.sw = sw = fe.sweep(name, kw, 1, salt)
        self.cfg = cfg = t3.make_cfg(mode=1, **kw)
        orc = ol.oracle()
        self.layouts, self.errs, self.streams, self.padded = [], [], [], []
        for i, W in enumerate(sw.Ws):
            clean = sw.stream("rgb", i)
            L = t3.plan(W, cfg)
            errs = [rp.schedule(int(L.band_k[b]), int(L.band_blocks[b]), i % 2)[0] for b in range(9)]
            bad = u8(rp.apply(orc, clean.reshape(-1, 9), L, sw.ocfg, errs))
            assert W == 0 or (bad != clean).any(), (name, W)
            bad.setflags(write=False)
            px = np.zeros(2 * W, ol.PIXEL_DT); px[: sw.n_px[i]] = sw.px[i]
            px.setflags(write=False)
            self.layouts.append(L); self.errs.append(errs); self.streams.append(bad); self.padded.append(px)
        first = next(i for i, W in enumerate(sw.Ws) if W > 1000)
        assert np.array_equal(orc.unpack_words(orc.pack_pixels(self.padded[first])), self.padded[first]), "the frames are in range: the packing keeps them"

    def far(self, i):
        """Frame i's schedule with a far row in the last block of band 8 (None: band 8 holds no block)."""
        L = self.layouts[i]
        if int(L.band_blocks[8]) == 0:
            return None
        errs = list(self.errs[i])
        pool = rp.far_errors(int(L.band_k[8]))
        errs[8] = errs[8].copy(); errs[8][-1] = pool[(i // FAR_EVERY) % len(pool)]
        return u8(rp.apply(ol.oracle(), self.sw.stream("rgb", i).reshape(-1, 9), L, self.sw.ocfg, errs))


@functools.lru_cache(maxsize=3)
def corrupted(name, salt=0):
    import __graft_entry__ as ge
    return Corrupted(ge.load_package(), name, salt)


def run_fixed_decoders(gpu, co, i, coded, outputs, rgb, far_rows, label):
    """One stream of frame i through t3hip_decode_frame_async (pixels / raw words) and t3hip_decode_rgb_async (the frame's own pixel
    count): capacity exactly the frame's, output and verdict words guarded, both fills; the launches of a fill are queued on one stream
    and checked after one synchronise.  far_rows > 0: the verdict counts them, the output is held to its guards only."""
    W, n_px, padded = co.sw.Ws[i], co.sw.n_px[i], co.padded[i]
    orc = ol.oracle(); s = stream()
    want = {True: u8(padded), False: u8(orc.pack_pixels(padded))}
    verdict = np.array([0, far_rows], np.uint32).view(np.uint8)
    n_in = len(coded) // 9
    for fill in bounds.FILLS:
        src = bounds.Buf(0, fill, 0, data=coded, name="%s coded input" % (label,))
        jobs = []
        for to_pixels in outputs:
            n, sz = (2 * W, 6) if to_pixels else (W, 9)
            what = "%s %s" % (label, "pixels" if to_pixels else "raw words")
            out = bounds.Buf(n * sz, fill, 0, name=what + " output"); ver = bounds.Buf(8, fill, 0, name=what + " verdict words")
            got = gpu.decode_frame_async(src.ptr, n_in, co.cfg, W, out.ptr, n, ver.ptr, to_pixels, s)
            assert got == n, (what, got, n)
            jobs.append((out, ver, want[to_pixels]))
        if rgb:
            out = bounds.Buf(3 * n_px, fill, 0, name="%s rgb output" % (label,)); ver = bounds.Buf(8, fill, 0, name="%s rgb verdict words" % (label,))
            gpu.decode_rgb_async(src.ptr, n_in, co.cfg, n_px, out.ptr, ver.ptr, s)
            jobs.append((out, ver, orc.quant_to_rgb(padded[:n_px])))
        bounds.sync()
        for out, ver, w in jobs:
            ver.expect(verdict)
            if far_rows:
                out.result()
            else:
                out.expect(w)
        src.result()


def one_code_1d_no_beacon(name):
    return name in rp.ONE_K


def sweep_fixed_decoders(gpu, name, outputs, label, with_far):
    co = corrupted(name)
    rgb = one_code_1d_no_beacon(name)
    for i, W in enumerate(co.sw.Ws):
        if W == 0:
            continue                                                          # (no frame: the decode entries take n_raw_words >= 1)
        run_fixed_decoders(gpu, co, i, co.streams[i], outputs, rgb, 0, (label, W, "schedule"))
        if with_far and i % FAR_EVERY == 0:
            run_fixed_decoders(gpu, co, i, co.sw.stream("rgb", i), outputs, rgb, 0, (label, W, "clean"))
            far = co.far(i)
            if far is not None:
                run_fixed_decoders(gpu, co, i, far, outputs, rgb, 1, (label, W, "far row"))


@pytest.mark.parametrize("name", list(rp.CONFIGS))
def test_fixed_decoders_at_every_frame_end(gpu, orc, name):
    """Every framing of rs_patterns.CONFIGS (fused kernel with and without a beacon in its loads, one-launch UEP / 2-D kernel, two-kernel
    decoder), pixels and -- where test_gpu_fixed_errors.OUTPUTS lists them -- raw words, RGB for the one-code 1-D framings without a beacon:
    the schedule stream of every lattice frame decodes to the frame zero-padded to 2 W pixels with verdict [0, 0]; every 10th frame also
    clean, and with one far row in the last block of band 8: verdict [0, 1]."""
    sweep_fixed_decoders(gpu, name, OUTPUTS[name], name, True)


@pytest.mark.parametrize("knob,name", KNOBS)
def test_fixed_decoders_forced_paths_at_every_frame_end(gpu, orc, knob, name):
    """The generic gather decoder and the two-kernel decoder forced by their knobs, on the same schedule streams."""
    os.environ[knob] = "1"
    try:
        sweep_fixed_decoders(gpu, name, OUTPUTS[name], "%s %s" % (knob, name), False)
    finally:
        os.environ.pop(knob, None)


@pytest.mark.parametrize("name", rp.ONE_K)
def test_batched_decode_at_every_frame_end(gpu, orc, name):
    """t3hip_decode_frames_async, three different frames per lattice size with the schedule's errors in each, pixels and RGB out, strides
    minimal and + 4112 in turn: every frame is its own original (and the oracle's quant_to_rgb of it), every verdict word 0, one launch."""
    cos = [corrupted(name, salt) for salt in (0, 1, 2)]
    cfg = cos[0].cfg
    for i, W in enumerate(cos[0].sw.Ws):
        if W == 0:
            continue
        coded = [c.streams[i] for c in cos]
        extra = STRIDE_EXTRA if i % 2 else 0
        for fmt in (gpu.FRAMES_PIXELS, gpu.FRAMES_RGB):
            p, seen, out, ver = decode_batch(gpu, coded, W, fmt, cfg, extra)
            assert p.one_launch == 1 and ver == [0] * 6, (name, W, fmt, ver)
            for f, c in enumerate(cos):
                want = u8(c.padded[i]) if fmt == gpu.FRAMES_PIXELS else orc.quant_to_rgb(c.padded[i])
                assert np.array_equal(seen[f], coded[f]) and np.array_equal(out[f], want), (name, W, fmt, "frame %d" % f)


@pytest.mark.parametrize("name", rp.ONE_K)
def test_window_decode_at_every_frame_end(gpu, orc, name):
    """t3hip_decode_window_async on the frame read as rows of 64 pixels: the rows that hold the frame's last 200 pixels and one row more.
    The window runs past the stream's end: pixels behind the end are zero records.  Pixels and RGB out, guarded, both fills."""
    co = corrupted(name)
    s = stream()
    for i, W in enumerate(co.sw.Ws):
        if W == 0:
            continue
        n = 2 * W; coded = co.streams[i]
        y0 = max(n - WINDOW_TAIL, 0) // WINDOW_FW
        h = -(-n // WINDOW_FW) - y0 + 1
        win = (WINDOW_FW, y0 + h, 0, y0, WINDOW_FW, h)
        assert y0 * WINDOW_FW <= max(n - WINDOW_TAIL, 0) and (y0 + h) * WINDOW_FW >= n + WINDOW_FW
        want_px = crop_np(co.padded[i], *win)
        want = {gpu.WINDOW_PIXELS: u8(want_px), gpu.WINDOW_RGB: orc.quant_to_rgb(want_px)}
        for fill in bounds.FILLS:
            src = bounds.Buf(0, fill, 0, data=coded, name="%s coded input" % ((name, W),))
            jobs = []
            for fmt, sz in ((gpu.WINDOW_PIXELS, 6), (gpu.WINDOW_RGB, 3)):
                out = bounds.Buf(WINDOW_FW * h * sz, fill, 0, name="%s window, format %d" % ((name, W), fmt)); ver = bounds.Buf(8, fill, 0, name="verdict words")
                gpu.decode_window_async(src.ptr, len(coded) // 9, co.cfg, W, *win, out.ptr, fmt, ver.ptr, s)
                jobs.append((out, ver, want[fmt]))
            bounds.sync()
            for out, ver, w in jobs:
                ver.expect(np.zeros(8, np.uint8)); out.expect(w)
            src.result()
