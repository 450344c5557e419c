"""GPU tests of the batched window / image entries (t3hip_decode_frames_window_async, t3hip_decode_frames_window,
t3hip_decode_images_async, t3hip_encode_images_dev; include/t3hip.h): byte for byte against the oracle's full decode + a numpy crop
(+ its quant_to_rgb) and against a loop of the single-frame entries.  Shapes are the smallest at which this can go wrong: a decoder tile
is 108 k pixels (2160 at k = 20), a frame of 100 x 70 = 7000 pixels is three or four tiles, the last one ragged, and three frames are an
odd count, so a workgroup's consecutive tickets cross frames.  Every output buffer carries 0xA5 guard bytes in front, behind and in the
stride gaps, checked after the call."""
import json
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as ol
from test_gpu_window import SINGLE, WHOLE, coded_frame, compose_np, crop_np
from test_window_plan import centered_window, units_tile

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K_OF = {0: 24, 1: 22, 2: 20, 3: 18}
NPX = 7000
# (fw, fh, x0, y0, w, h) on a stream of 100 x 70 pixels
WINS = [
    (100, 70, 0, 0, 100, 70),      # the whole frame
    (100, 70, 10, 22, 50, 20),     # at k = 20 starts in tile 1
    (100, 70, 3, 44, 1, 1),        # tile 2 only
    (100, 70, 37, 65, 63, 5),      # the ragged last tile
    (100, 80, 0, 60, 100, 20),     # rows past the stream
    (98, 72, 5, 1, 91, 3),         # fw * fh is not the pixel count; odd x0 and w
    (100, 70, 0, 90, 10, 10),      # wholly behind the stream: the loop path
]
GUARD = 256
E_HEADER, E_RS = -5, -6                            # include/t3hip.h; the oracle answers with the same codes


def r16(x):
    return (x + 15) & ~15


def ubytes(gpu, fmt):
    return 6 if fmt == gpu.WINDOW_PIXELS else 3


class Batch:
    """n coded frames of one configuration in one device buffer at stride minimum + extra, and the streams on the host."""

    def __init__(self, gpu, frames, extra=48, host=True):
        import torch
        self.n = len(frames); self.n_enc, self.cfg, self.L = frames[0][1], frames[0][2], frames[0][3]
        self.stride = r16(9 * self.n_enc) + extra
        self.buf = torch.zeros(self.n * self.stride + 64, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 16 == 0
        for f, fr in enumerate(frames):
            assert fr[1] == self.n_enc
            self.buf[f * self.stride: f * self.stride + 9 * self.n_enc] = fr[0][: 9 * self.n_enc]
        torch.cuda.synchronize()
        if host:
            self.refresh()

    def refresh(self):
        host = self.buf.cpu().numpy()
        self.streams = [host[f * self.stride: f * self.stride + 9 * self.n_enc].copy() for f in range(self.n)]

    def frame_ptr(self, f):
        return self.buf.data_ptr() + f * self.stride


def make_batch(gpu, orc, kw, n, n_px, max_err, extra=48):
    """n frames of LCG pixels (seeds 12345 + f), encoded on the device, 0..max_err symbol errors per block (a seed per frame)"""
    return Batch(gpu, [coded_frame(gpu, orc, kw, n_px, 12345 + f, max_err) for f in range(n)], extra)


def batch_window(gpu, b, n_raw, win, fmt, extra=0, n=None, first=0):
    """The batched call on frames [first, first + n) -> ([window bytes per frame], verdict words); guards checked."""
    import torch
    n = b.n if n is None else n
    fw, fh, x0, y0, w, h = win
    nb = w * h * ubytes(gpu, fmt); stride = r16(nb) + extra
    buf = torch.full((2 * GUARD + max(n, 1) * stride,), 0xA5, dtype=torch.uint8, device="cuda")
    ver = torch.full((2 * n + 2,), 7, dtype=torch.int32, device="cuda")
    assert (buf.data_ptr() + GUARD) % 16 == 0
    gpu.decode_frames_window_async(b.frame_ptr(first), b.n_enc, b.stride, n, b.cfg, n_raw, fw, fh, x0, y0, w, h, buf.data_ptr() + GUARD, stride, fmt, ver.data_ptr(),
                                   torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    host = buf.cpu().numpy(); v = ver.cpu().tolist()
    assert (host[:GUARD] == 0xA5).all() and (host[GUARD + n * stride:] == 0xA5).all(), "wrote outside the batch's output"
    for f in range(n):
        assert (host[GUARD + f * stride + nb: GUARD + (f + 1) * stride] == 0xA5).all(), "wrote into the stride gap behind frame %d" % f
    assert v[2 * n:] == [7, 7], "wrote behind the verdict words"
    return [host[GUARD + f * stride: GUARD + f * stride + nb] for f in range(n)], v[: 2 * n]


def single_window(gpu, b, f, n_raw, win, fmt):
    """decode_window_async on frame f of the batch -> (bytes, verdict words); guards checked"""
    import torch
    fw, fh, x0, y0, w, h = win
    nb = w * h * ubytes(gpu, fmt)
    buf = torch.full((2 * GUARD + nb,), 0xA5, dtype=torch.uint8, device="cuda"); ver = torch.full((2,), 7, dtype=torch.int32, device="cuda")
    gpu.decode_window_async(b.frame_ptr(f), b.n_enc, b.cfg, n_raw, fw, fh, x0, y0, w, h, buf.data_ptr() + GUARD, fmt, ver.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[:GUARD] == 0xA5).all() and (host[GUARD + nb:] == 0xA5).all()
    return host[GUARD: GUARD + nb], ver.cpu().tolist()


def want_bytes(gpu, orc, px, win, fmt):
    c = crop_np(px, *win)
    return c.view(np.uint8) if fmt == gpu.WINDOW_PIXELS else orc.quant_to_rgb(c)


def one_launch_rule(p, n, win):
    return 1 if (p.win.tile_range == 1 and p.win.tile_hi > p.win.tile_lo and n >= 2 and win[4] * win[5]) else 0


def windows_for(gpu, cfg, k):
    """WINS, plus a one-pixel window at the start of tile r for every r in 0..2 that no window's range starts at (mod 3): the
    scrambler phase of a tile is (tile * 52) mod 3 = tile mod 3."""
    wins = list(WINS)
    seen = {gpu.window_plan(NPX // 2, cfg, *w).tile_lo % 3 for w in wins if gpu.window_plan(NPX // 2, cfg, *w).tile_hi > gpu.window_plan(NPX // 2, cfg, *w).tile_lo}
    for r in sorted({0, 1, 2} - seen):
        p0 = r * units_tile(k)
        wins.append((100, 70, p0 % 100, p0 // 100, 1, 1))
    lo = {gpu.window_plan(NPX // 2, cfg, *w).tile_lo % 3 for w in wins if gpu.window_plan(NPX // 2, cfg, *w).tile_hi > gpu.window_plan(NPX // 2, cfg, *w).tile_lo}
    assert lo == {0, 1, 2}, (k, lo)
    return wins


_cache = {}


def small_batch(gpu, orc, name, max_err):
    """3 frames of 100 x 70 in the code `name` and the oracle's decode of each (corrupted) stream, made once per module"""
    key = (name, max_err)
    if key not in _cache:
        b = make_batch(gpu, orc, SINGLE[name], 3, NPX, max_err)
        px = []
        for f in range(3):
            rc, p = orc.decode_frame(b.streams[f], ol.make_cfg(mode=1, **SINGLE[name]))
            assert rc == 0 and len(p) == NPX
            px.append(p)
        _cache[key] = (b, px)
    return _cache[key]


@pytest.mark.parametrize("name", sorted(SINGLE))
def test_against_the_oracle(gpu, orc, name):
    """Four codes, 0 and t errors per block, in-stride minimum + 48, out-stride minimum and minimum + 32, both formats: every frame's window
    equals the oracle's decode of that frame's stream, cropped in numpy (and its quant_to_rgb); verdicts all zero; the plan's one_launch as
    the rule says; the ranges start at tiles = 0, 1 and 2 mod 3."""
    k = K_OF[SINGLE[name]["profile"]]; n_raw = NPX // 2
    for max_err in (0, (26 - k) // 2):
        b, px = small_batch(gpu, orc, name, max_err)
        for win in windows_for(gpu, b.cfg, k):
            for fmt in (gpu.WINDOW_PIXELS, gpu.WINDOW_RGB):
                p = gpu.frames_window_plan(n_raw, 3, b.cfg, *win, fmt)
                assert p.one_launch == one_launch_rule(p, 3, win) == (0 if win[3] >= 70 else 1), (name, win)
                for extra in (0, 32):
                    got, ver = batch_window(gpu, b, n_raw, win, fmt, extra)
                    assert ver == [0, 0] * 3, (name, max_err, win, fmt, ver)
                    for f in range(3):
                        assert np.array_equal(got[f], want_bytes(gpu, orc, px[f], win, fmt)), (name, max_err, win, fmt, extra, f)


@pytest.mark.parametrize("name", sorted(SINGLE))
def test_against_the_loop(gpu, orc, name):
    """Output and verdict words equal a loop of decode_window_async over the frames, for every window and format.  One frame: the
    single-frame entry (any stride).  No frame: nothing is written."""
    import torch
    k = K_OF[SINGLE[name]["profile"]]; n_raw = NPX // 2
    b, _ = small_batch(gpu, orc, name, (26 - k) // 2)
    for win in windows_for(gpu, b.cfg, k):
        for fmt in (gpu.WINDOW_PIXELS, gpu.WINDOW_RGB):
            got, ver = batch_window(gpu, b, n_raw, win, fmt, 16)
            for f in range(3):
                one, v1 = single_window(gpu, b, f, n_raw, win, fmt)
                assert np.array_equal(got[f], one) and ver[2 * f: 2 * f + 2] == v1, (name, win, fmt, f)
            g1, v = batch_window(gpu, b, n_raw, win, fmt, 0, n=1, first=2)
            one, v1 = single_window(gpu, b, 2, n_raw, win, fmt)
            assert np.array_equal(g1[0], one) and v == v1
            g0, v = batch_window(gpu, b, n_raw, win, fmt, 0, n=0)                      # (the guards: nothing written at all)
            assert g0 == [] and v == []
    # an empty window: T3_OK, nothing launched, verdicts untouched
    for (w, h) in [(0, 9), (9, 0)]:
        got, ver = batch_window(gpu, b, n_raw, (100, 70, 5, 5, w, h), gpu.WINDOW_RGB, 16)
        assert ver == [7] * 6
    # another configuration's header: every frame's verdict[0]; a truncated stream: T3_E_HEADER
    other = gpu.make_cfg(mode=1, seed=(1, 1, 2), **SINGLE[name])
    out = torch.full((3 * 4096,), 0xA5, dtype=torch.uint8, device="cuda"); ver = torch.full((6,), 7, dtype=torch.int32, device="cuda")
    gpu.decode_frames_window_async(b.frame_ptr(0), b.n_enc, b.stride, 3, other, n_raw, 100, 70, 10, 22, 50, 10, out.data_ptr(), 3008, gpu.WINDOW_PIXELS, ver.data_ptr())
    torch.cuda.synchronize()
    assert ver.cpu().tolist()[0::2] == [1, 1, 1]
    with pytest.raises(gpu.T3Error) as e:
        gpu.decode_frames_window_async(b.frame_ptr(0), b.n_enc - 5, b.stride, 3, b.cfg, n_raw, 100, 70, 10, 22, 50, 10, out.data_ptr(), 3008, gpu.WINDOW_PIXELS, ver.data_ptr())
    assert e.value.code == gpu.E_HEADER


def test_more_tickets_than_workgroups(gpu, orc):
    """16 frames of 960 x 540, k = 20, 0..3 errors per block: n_frames * (tile_hi - tile_lo) >= 1024 tickets, above the resident grid (at
    most three workgroups on each of 256 CUs), so the tickets cycle.  Against the loop of the single-frame entry; frames 0 and 15 against
    the oracle."""
    n, n_px = 16, 960 * 540; n_raw = n_px // 2
    win = (960, 540, 100, 200, 300, 150)
    b = make_batch(gpu, orc, SINGLE["p3_k20"], n, n_px, 3)
    p = gpu.frames_window_plan(n_raw, n, b.cfg, *win, gpu.WINDOW_RGB)
    assert p.one_launch == 1 and n * (p.win.tile_hi - p.win.tile_lo) >= 1024
    px = {f: orc.decode_frame(b.streams[f], ol.make_cfg(mode=1, **SINGLE["p3_k20"])) for f in (0, 15)}
    assert all(rc == 0 and len(v) == n_px for rc, v in px.values())
    for fmt in (gpu.WINDOW_PIXELS, gpu.WINDOW_RGB):
        got, ver = batch_window(gpu, b, n_raw, win, fmt, 32)
        assert ver == [0, 0] * n
        for f in range(n):
            one, v1 = single_window(gpu, b, f, n_raw, win, fmt)
            assert v1 == [0, 0] and np.array_equal(got[f], one), (fmt, f)
        for f in (0, 15):
            assert np.array_equal(got[f], want_bytes(gpu, orc, px[f][1], win, fmt)), (fmt, f)


def damage_block(orc, stream, L, ocfg, block, n_bad):
    """n_bad symbols of block `block` of band 0 altered to other values in 0..26 so that the oracle calls the block uncorrectable
    (t + 1 errors land within t of another codeword now and then: the first pattern of offsets that does not)."""
    at = int(L.header_syms) + int(L.band_body_off[0]) + 26 * block
    for step in range(26):
        cand = stream.copy()
        for i in range(n_bad):
            cand[at + i] = (int(cand[at + i]) + 1 + (step + 5 * i) % 26) % 27                   # + 1..26: never the value it had
        assert all(cand[at + i] != stream[at + i] and cand[at + i] < 27 for i in range(n_bad))
        if orc.decode_frame(cand, ocfg)[0] == E_RS:
            return cand
    raise AssertionError("no pattern gave an uncorrectable block")


def test_damage_stays_in_its_frame(gpu, orc):
    """k = 20, a window that covers tiles 1..2 only.  Frame 1: t + 1 altered symbols in a block of tile 1 -> its block count, not its header
    word, and nothing of its neighbours.  Frame 2: the same damage in a block of tile 0, which the window does not cover: not decoded, not
    reported, the window right.  Then the host entry: per-frame codes, a correctable header symbol (the redo path), an undecodable header."""
    import torch
    name = "p3_k20"; n_raw = NPX // 2; win = (100, 70, 0, 22, 100, 42); ocfg = ol.make_cfg(mode=1, **SINGLE[name])
    b = make_batch(gpu, orc, SINGLE[name], 3, NPX, 0)
    p = gpu.frames_window_plan(n_raw, 3, b.cfg, *win)
    assert (p.win.tile_lo, p.win.tile_hi, p.one_launch) == (1, 3, 1)
    clean = [s.copy() for s in b.streams]
    px = [orc.decode_frame(s, ocfg)[1] for s in clean]
    bad1 = damage_block(orc, clean[1], b.L, ocfg, 60, 4)                                  # tile 1 holds blocks 52..103 of every band
    bad2 = damage_block(orc, clean[2], b.L, ocfg, 5, 4)                                   # tile 0
    assert orc.decode_frame(bad1, ocfg)[0] == E_RS                                    # the input condition: the oracle alone gives frame 1 up
    for f, s in ((1, bad1), (2, bad2)):
        b.buf[f * b.stride: f * b.stride + len(s)] = torch.from_numpy(s).cuda()
    torch.cuda.synchronize(); b.refresh()
    for fmt in (gpu.WINDOW_PIXELS, gpu.WINDOW_RGB):
        got, ver = batch_window(gpu, b, n_raw, win, fmt, 16)
        assert ver[2] == 0 and ver[3] >= 1, ver
        assert ver[0:2] == [0, 0] and ver[4:6] == [0, 0], ver
        assert np.array_equal(got[0], want_bytes(gpu, orc, px[0], win, fmt))
        assert np.array_equal(got[2], want_bytes(gpu, orc, px[2], win, fmt))
    # the host entry
    hdr1 = b.streams[0].copy(); hdr1[5] = (int(hdr1[5]) + 1) % 27                          # one header symbol: RS(26,18) corrects it
    assert orc.decode_frame(hdr1, ocfg)[0] == 0
    rcs, wins = gpu.decode_frames_window([hdr1, b.streams[1], b.streams[2]], b.cfg, n_raw, *win, gpu.WINDOW_PIXELS)
    assert rcs == [gpu.OK, gpu.E_RS, gpu.OK], rcs
    assert np.array_equal(wins[0].view(np.uint8), want_bytes(gpu, orc, px[0], win, gpu.WINDOW_PIXELS))
    assert np.array_equal(wins[2].view(np.uint8), want_bytes(gpu, orc, px[2], win, gpu.WINDOW_PIXELS))
    hdr10 = b.streams[0].copy(); hdr10[:10] = (hdr10[:10].astype(np.int64) + 1) % 27       # ten symbols of header block 0: beyond t = 4
    assert orc.decode_frame(hdr10, ocfg)[0] == E_HEADER
    rcs, wins = gpu.decode_frames_window([hdr10, b.streams[1], b.streams[2]], b.cfg, n_raw, *win, gpu.WINDOW_RGB)
    assert rcs == [gpu.E_HEADER, gpu.E_RS, gpu.OK], rcs
    assert len(wins[0]) == 0 and np.array_equal(wins[2].reshape(-1), want_bytes(gpu, orc, px[2], win, gpu.WINDOW_RGB))


@pytest.mark.parametrize("name", sorted(WHOLE))
def test_per_frame_framings(gpu, orc, name):
    """Per-band k, 2-D and beacon frames: the plan is the loop, the bytes and words equal the loop's and the oracle's."""
    n_raw = NPX // 2; ocfg = ol.make_cfg(mode=1, **WHOLE[name])
    b = make_batch(gpu, orc, WHOLE[name], 2, NPX, 1)
    px = []
    for f in range(2):
        rc, p = orc.decode_frame(b.streams[f], ocfg)
        assert rc == 0 and len(p) == NPX
        px.append(p)
    for win in (WINS[1], WINS[4]):
        for fmt in (gpu.WINDOW_PIXELS, gpu.WINDOW_RGB):
            assert gpu.frames_window_plan(n_raw, 2, b.cfg, *win, fmt).one_launch == 0
            got, ver = batch_window(gpu, b, n_raw, win, fmt, 16)
            assert ver == [0, 0] * 2
            for f in range(2):
                one, v1 = single_window(gpu, b, f, n_raw, win, fmt)
                assert np.array_equal(got[f], one) and v1 == [0, 0]
                assert np.array_equal(got[f], want_bytes(gpu, orc, px[f], win, fmt)), (name, win, fmt, f)


def image_frames(gpu, orc, n, sw, sh, sub, centered, cfg, extra=48, host=True):
    """n sources of sw x sh (LCG RGB, seeds 40 + f) -> (sources, [coded frame tensors by encode_image_dev], n_enc, in a Batch)"""
    import torch
    s = torch.cuda.current_stream().cuda_stream
    fw, fh = gpu.image_geometry(sub, centered)[:2]
    n_enc = gpu.encoded_words(fw * fh // 2, cfg)
    srcs = [orc.lcg_rgb(sw * sh, 40 + f).reshape(sh, sw, 3) for f in range(n)]
    frames = []
    for src in srcs:
        d = torch.from_numpy(src.reshape(-1)).cuda(); out = torch.zeros(n_enc * 9 + 64, dtype=torch.uint8, device="cuda")
        assert gpu.encode_image_dev(d.data_ptr(), sw, sh, sub, centered, cfg, out.data_ptr(), n_enc, s) == n_enc
        torch.cuda.synchronize()
        frames.append((out, n_enc, cfg, None))
    return srcs, Batch(gpu, frames, extra, host)


def images_of(gpu, b, sub, centered, extra):
    """decode_images_async on the batch -> device tensor of the images (guards checked on the device), stride, bytes, verdicts"""
    import torch
    tw, th = gpu.image_geometry(sub, centered)[4:]
    nb = tw * th * 3; stride = r16(nb) + extra
    buf = torch.full((2 * GUARD + b.n * stride,), 0xA5, dtype=torch.uint8, device="cuda"); ver = torch.full((2 * b.n + 2,), 7, dtype=torch.int32, device="cuda")
    gpu.decode_images_async(b.frame_ptr(0), b.n_enc, b.stride, b.n, b.cfg, sub, centered, buf.data_ptr() + GUARD, stride, ver.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert bool((buf[:GUARD] == 0xA5).all()) and bool((buf[GUARD + b.n * stride:] == 0xA5).all())
    for f in range(b.n):
        assert bool((buf[GUARD + f * stride + nb: GUARD + (f + 1) * stride] == 0xA5).all())
    v = ver.cpu().tolist()
    assert v[2 * b.n:] == [7, 7]
    return [buf[GUARD + f * stride: GUARD + f * stride + nb] for f in range(b.n)], v[: 2 * b.n]


def image_loop(gpu, b, f, sub, centered):
    import torch
    tw, th = gpu.image_geometry(sub, centered)[4:]
    rgb = torch.full((tw * th * 3 + 64,), 0xA5, dtype=torch.uint8, device="cuda"); ver = torch.full((2,), 7, dtype=torch.int32, device="cuda")
    gpu.decode_image_async(b.frame_ptr(f), b.n_enc, b.cfg, sub, centered, rgb.data_ptr(), ver.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rgb[: tw * th * 3], ver.cpu().tolist()


def test_decode_images(gpu, orc):
    """decode_images_async, S15 not centred (854 x 480 frames made by encode_image_dev from 100 x 75 sources), 3 frames: against the
    oracle's decode + quant_to_rgb and against the loop of decode_image_async."""
    import torch
    cfg = gpu.make_cfg(mode=1, profile=2, uep=2); ocfg = ol.make_cfg(mode=1, profile=2, uep=2)
    srcs, b = image_frames(gpu, orc, 3, 100, 75, 15, False, cfg)
    assert gpu.frames_window_plan(854 * 480 // 2, 3, cfg, 854, 480, 0, 0, 854, 480, gpu.WINDOW_RGB).one_launch == 1
    want = []
    for f in range(3):
        rc, px = orc.decode_frame(b.streams[f], ocfg)
        assert rc == 0 and len(px) == 854 * 480
        want.append(orc.quant_to_rgb(px))
    for extra in (0, 32):
        got, ver = images_of(gpu, b, 15, False, extra)
        assert ver == [0, 0] * 3
        for f in range(3):
            assert np.array_equal(got[f].cpu().numpy(), want[f]), f
            one, v1 = image_loop(gpu, b, f, 15, False)
            assert v1 == [0, 0] and bool(torch.equal(got[f], one)), f


def test_decode_images_8k_centred(gpu, orc):
    """S21 centred (1920 x 1080 inside 7680 x 4320), 2 frames: against the loop of decode_image_async only -- the oracle needs minutes for
    an 8K frame; the single-frame entry is held to the oracle at this size by test_gpu_window.test_window_decode_8k."""
    import torch
    cfg = gpu.make_cfg(mode=1, profile=2, uep=2)
    srcs, b = image_frames(gpu, orc, 2, 100, 75, 21, True, cfg, host=False)
    x0, y0, w, h = centered_window(21)
    p = gpu.frames_window_plan(7680 * 4320 // 2, 2, cfg, 7680, 4320, x0, y0, w, h, gpu.WINDOW_RGB)
    assert p.one_launch == 1 and 0 < p.win.tile_lo < p.win.tile_hi < p.win.n_tiles
    got, ver = images_of(gpu, b, 21, True, 16)
    assert ver == [0, 0] * 2
    for f in range(2):
        one, v1 = image_loop(gpu, b, f, 21, True)
        assert v1 == [0, 0] and bool(torch.equal(got[f], one)), f


def encode_images(gpu, srcs, sub, centered, cfg, extra_out=32):
    """encode_images_dev on sources packed at stride minimum + 5 (odd source addresses) -> ([coded frame tensors], n_enc); guards checked"""
    import torch
    n = len(srcs); sh, sw = srcs[0].shape[:2]
    fw, fh = gpu.image_geometry(sub, centered)[:2]
    n_enc = gpu.encoded_words(fw * fh // 2, cfg)
    sstride = sw * sh * 3 + 5
    src = torch.zeros(n * sstride + 16, dtype=torch.uint8, device="cuda")
    for f, a in enumerate(srcs):
        src[f * sstride: f * sstride + sw * sh * 3] = torch.from_numpy(a.reshape(-1)).cuda()
    nb = 9 * n_enc; stride = r16(nb) + extra_out
    out = torch.full((2 * GUARD + n * stride,), 0xA5, dtype=torch.uint8, device="cuda")
    assert (out.data_ptr() + GUARD) % 16 == 0
    assert gpu.encode_images_dev(src.data_ptr(), sw, sh, sstride, n, sub, centered, cfg, out.data_ptr() + GUARD, stride, torch.cuda.current_stream().cuda_stream) == n_enc
    torch.cuda.synchronize()
    assert bool((out[:GUARD] == 0xA5).all()) and bool((out[GUARD + n * stride:] == 0xA5).all())
    for f in range(n):
        assert bool((out[GUARD + f * stride + nb: GUARD + (f + 1) * stride] == 0xA5).all())
    return [out[GUARD + f * stride: GUARD + f * stride + nb] for f in range(n)], n_enc


def encode_image_loop(gpu, src, sub, centered, cfg, n_enc):
    import torch
    sh, sw = src.shape[:2]
    d = torch.from_numpy(src.reshape(-1)).cuda(); out = torch.zeros(n_enc * 9 + 64, dtype=torch.uint8, device="cuda")
    assert gpu.encode_image_dev(d.data_ptr(), sw, sh, sub, centered, cfg, out.data_ptr(), n_enc, torch.cuda.current_stream().cuda_stream) == n_enc
    torch.cuda.synchronize()
    return out[: 9 * n_enc]


@pytest.mark.parametrize("sw,sh", [(100, 75), (854, 480)])
def test_encode_images(gpu, orc, sw, sh):
    """encode_images_dev, S15, 3 sources (a resize / none), sources at stride minimum + 5: every coded frame equals encode_image_dev on
    its source and the oracle's encode of the numpy compose, byte for byte."""
    import torch
    cfg = gpu.make_cfg(mode=1, profile=2, uep=2); ocfg = ol.make_cfg(mode=1, profile=2, uep=2)
    srcs = [orc.lcg_rgb(sw * sh, 60 + f).reshape(sh, sw, 3) for f in range(3)]
    got, n_enc = encode_images(gpu, srcs, 15, False, cfg)
    for f in range(3):
        assert bool(torch.equal(got[f], encode_image_loop(gpu, srcs[f], 15, False, cfg, n_enc))), f
        frame, _ = compose_np(orc, srcs[f], 15, False)
        rc, want = orc.encode_frame(orc.rgb_to_quant(np.ascontiguousarray(frame).reshape(-1)), ocfg)
        assert rc == 0 and np.array_equal(got[f].cpu().numpy(), want.reshape(-1)), f
    one, _ = encode_images(gpu, srcs[:1], 15, False, cfg)                                   # one frame: the single entry's bytes
    assert bool(torch.equal(one[0], got[0]))
    if sw == 100:                                                                            # no source pixels: zero frames composed, as the single entry does
        zero, _ = encode_images(gpu, [np.zeros((0, 0, 3), np.uint8)] * 2, 15, False, cfg)
        z1 = encode_image_loop(gpu, np.zeros((0, 0, 3), np.uint8), 15, False, cfg, n_enc)
        assert bool(torch.equal(zero[0], z1)) and bool(torch.equal(zero[1], z1))


def test_encode_images_8k_centred(gpu, orc):
    """S21 centred, 2 sources of 100 x 75, against the loop of encode_image_dev only (the oracle needs minutes for an 8K frame)."""
    import torch
    cfg = gpu.make_cfg(mode=1, profile=2, uep=2)
    srcs = [orc.lcg_rgb(100 * 75, 70 + f).reshape(75, 100, 3) for f in range(2)]
    got, n_enc = encode_images(gpu, srcs, 21, True, cfg)
    for f in range(2):
        assert bool(torch.equal(got[f], encode_image_loop(gpu, srcs[f], 21, True, cfg, n_enc))), f


def test_frames_window_demo(gpu, orc, tmp_path):
    """tests/cpp/frames_window_demo.cpp: images_to_frames, frames_to_images and decode_frames_window of include/ternary_codec_v6.hpp; frame
    1 of 3 carries 13 damaged symbols in a block of tile 0, which spoils its image and not its window further down."""
    lib = os.path.join(ROOT, "ternary-image-codec_amd"); exe = os.path.join(str(tmp_path), "frames_window_demo")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include", "compat"), "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "frames_window_demo.cpp"), "-L" + lib, "-lt3hip", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-o", exe], check=True)
    n, sw, sh, bad = 3, 100, 75, 1
    win = (854, 480, 301, 200, 333, 77)
    ocfg = ol.make_cfg(mode=1, profile=2, uep=2)
    srcs = [orc.lcg_rgb(sw * sh, 80 + f).reshape(sh, sw, 3) for f in range(n)]
    p = lambda name: os.path.join(str(tmp_path), name)
    np.concatenate([s.reshape(-1) for s in srcs]).tofile(p("in.rgb"))
    r = subprocess.run([exe, str(n), str(sw), str(sh), str(bad)] + [str(v) for v in win[2:]] + [p("in.rgb"), p("words"), p("rgb"), p("win")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    info = json.loads(r.stdout.strip().splitlines()[-1])
    want = []
    for s in srcs:
        frame, _ = compose_np(orc, s, 15, False)
        rc, w = orc.encode_frame(orc.rgb_to_quant(np.ascontiguousarray(frame).reshape(-1)), ocfg)
        assert rc == 0
        want.append(w.reshape(-1).copy())
    assert np.array_equal(np.fromfile(p("words"), np.uint8), np.concatenate(want))
    assert info["frames"] == n and info["words"] == len(want[0]) // 9 and info["uneven_refused"] == 1
    dead = want[bad].copy(); dead[90: 103] = (dead[90: 103] + 1) % 27
    assert orc.decode_frame(dead, ocfg)[0] == E_RS
    assert info["good_img"] == [1, 0, 1] and info["all_img"] == 0 and info["good_win"] == [1, 1, 1] and info["all_win"] == 1
    rgb = np.fromfile(p("rgb"), np.uint8).reshape(n, -1); wpx = np.fromfile(p("win"), ol.PIXEL_DT).reshape(n, -1)
    for f in range(n):
        rc, px = orc.decode_frame(want[f], ocfg)
        assert rc == 0
        assert np.array_equal(rgb[f], orc.quant_to_rgb(px) if f != bad else np.zeros(854 * 480 * 3, np.uint8)), f
        assert np.array_equal(wpx[f], crop_np(px, *win)), f
