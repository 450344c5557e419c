"""GPU tests of every frame decoder on received bytes 27..255.  A coded byte above 26 is no symbol; the contract (FIXED
section) is that every decoder takes it mod 27, as the oracle does, and steps over a beacon slot whatever it holds.  The device carries
that reduction four times, each behind a guard of its own: fx2_set (fused, fused-pixel, batch and one-launch UEP kernels), fx_block
(two-kernel decoder), sub_trits (generic decoder, FIXED and COMPAT) and the header (% 27 on the host; a byte compare on the device).

The streams are those of rs_patterns.lift -- dense / sparse lifting on top of the <= t schedule and of frames with far rows, every value
27..255 at every position on the clean stream, random beacon-slot bytes -- and every expectation is proven with the oracle alone in
test_noncanonical_semantics.py, which also shows that the same streams under a wrong reduction are refused or decode to other pixels.
Every device input holds its stream at a 256-byte boundary between two runs of >= 256 bytes of 0xFF: lanes without a block and the
over-reading loads of the kernels see high bytes that are not theirs.  Byte work: every comparison is exact."""
import os

import numpy as np
import pytest

import oracle_lib as ol
import rs_patterns as rp
import test_gpu_frames as tf
from test_gpu_fixed_errors import KNOBS, OUTPUTS, Dev, _frame, check_streams, expected
from test_noncanonical_semantics import COMPAT_NAMES, compat_streams, header_lifts

pytestmark = pytest.mark.gpu
GUARD, HIGH = 256, 0xFF
SIZES = ("full", "padded", "small")


class Guarded:
    """A stream on the device: at a 256-byte boundary, GUARD bytes of 0xFF in front of it, at least GUARD behind it."""

    def __init__(self, stream):
        import torch
        b = np.ascontiguousarray(stream, np.uint8).reshape(-1)
        buf = np.full(2 * GUARD + (len(b) + GUARD - 1) // GUARD * GUARD, HIGH, np.uint8)
        buf[GUARD: GUARD + len(b)] = b
        self.t, self.n = torch.from_numpy(buf).cuda(), len(b)
        assert self.data_ptr() % 256 == 0

    def data_ptr(self):
        return self.t.data_ptr() + GUARD

    def numel(self):
        return self.n


def lifted_on_device(orc, fr, what, only=None):
    """-> (case, Guarded stream, M, where, expected bytes or None) for every lifted stream of the frame (check_streams' input)"""
    for base, pattern in rp.lift_names(fr, what):
        if only is not None and (base, pattern) not in only:
            continue
        s, _, M, where = rp.lifted(fr, base, pattern)
        assert (s > 26).any() or (what == "small" and pattern == "sparse")      # (under 18 blocks a band `sparse` lifts nothing)
        yield "%s+%s" % (base, pattern), Guarded(s), M, where, expected(orc, fr, "sched" if M == 0 else "far", s)


# ---- a. every framing -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", SIZES)
@pytest.mark.parametrize("name", sorted(rp.CONFIGS))
def test_every_framing(gpu, orc, name, what):
    """All 13 framings at three sizes through t3hip_decode_frame_async and t3hip_decode_profile_dev, pixels and (where listed) raw words:
    verdict [0, 0] and the original frame; on top of M far rows [0, M], T3_E_RS, and the tiles without a far row still original."""
    fr = _frame(name, what)
    check_streams(gpu, Dev(gpu, fr), fr, lifted_on_device(orc, fr, what), OUTPUTS[name], what, name)


# ---- b. forced paths --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("knob,name", KNOBS)
def test_forced_paths(gpu, orc, knob, name):
    """The two-kernel decoder (fx_block) and the generic gather decoder (sub_trits) forced by their knobs."""
    fr = _frame(name, "full")
    os.environ[knob] = "1"
    try:
        check_streams(gpu, Dev(gpu, fr), fr, lifted_on_device(orc, fr, "full", (("sched", "dense"), ("clean", "values"))), (True,), "full", "%s %s" % (knob, name))
    finally:
        os.environ.pop(knob, None)


# ---- c. the other entry points ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", rp.ONE_K)
def test_other_entry_points(gpu, orc, name):
    """One k, 1-D: the window decode over the whole frame (tile-range plan, pixels and RGB) and over one interior window, whose verdict
    counts the far rows of its own tiles only; the RGB entry; the body entry (d_fail = M); the host entry, chunk by chunk at this size."""
    import torch
    fr = _frame(name, "full")
    dev = Dev(gpu, fr); n = dev.n_px; s = dev.s; k = fr.ks[0]
    assert -(-max(fr.blocks) // 52) >= 64
    rgb = torch.zeros(3 * n + 64, dtype=torch.uint8, device="cuda")
    fail = torch.zeros(1, dtype=torch.int32, device="cuda")
    x0, w = 2 * 108 * k + 37, 2 * 108 * k + 11                        # tiles 2, 3 and 4
    wp = gpu.window_plan(fr.n_raw, dev.cfg, n, 1, x0, 0, w, 1)
    assert gpu.window_plan(fr.n_raw, dev.cfg, n, 1, 0, 0, n, 1).tile_range == 1 and (wp.tile_range, wp.tile_lo, wp.tile_hi) == (1, 2, 5)
    for case, d, M, where, want in lifted_on_device(orc, fr, "full"):
        label = (name, case)
        for fmt, size in ((gpu.WINDOW_PIXELS, 6), (gpu.WINDOW_RGB, 3)):
            dev.out.fill_(0xA5); dev.ver.fill_(7)
            gpu.decode_window_async(d.data_ptr(), d.numel() // 9, dev.cfg, fr.n_raw, n, 1, 0, 0, n, 1, dev.out.data_ptr(), fmt, dev.ver.data_ptr(), s)
            torch.cuda.synchronize()
            assert dev.ver.cpu().tolist() == [0, M], (label, fmt)
            if want is not None:
                px = want[True].view(ol.PIXEL_DT)
                assert np.array_equal(dev.out[: n * size].cpu().numpy(), want[True] if size == 6 else orc.quant_to_rgb(px)), (label, fmt)
        inside = sum(1 for (_, m) in where if 2 <= m // 52 < 5)
        dev.out.fill_(0xA5); dev.ver.fill_(7)
        gpu.decode_window_async(d.data_ptr(), d.numel() // 9, dev.cfg, fr.n_raw, n, 1, x0, 0, w, 1, dev.out.data_ptr(), gpu.WINDOW_PIXELS, dev.ver.data_ptr(), s)
        torch.cuda.synchronize()
        assert dev.ver.cpu().tolist() == [0, inside], (label, "interior window")
        if inside == 0:
            assert np.array_equal(dev.out[: 6 * w].cpu().numpy(), fr.padded[x0: x0 + w].view(np.uint8)), (label, "interior window")
        assert bool((dev.out[6 * w: 6 * w + 64] == 0xA5).all()), (label, "interior window")
        rgb.fill_(0xA5); dev.ver.fill_(7)
        gpu.decode_rgb_async(d.data_ptr(), d.numel() // 9, dev.cfg, n, rgb.data_ptr(), dev.ver.data_ptr(), s)
        torch.cuda.synchronize()
        assert dev.ver.cpu().tolist() == [0, M], (label, "rgb")
        if want is not None:
            assert np.array_equal(rgb[: 3 * n].cpu().numpy(), orc.quant_to_rgb(want[True].view(ol.PIXEL_DT))), (label, "rgb")
        dev.out.fill_(0xA5); fail.zero_()
        got = gpu.decode_body_dev(d.data_ptr(), d.numel() // 9, dev.cfg, fr.n_raw, dev.out.data_ptr(), n, fail.data_ptr(), True, s)
        torch.cuda.synchronize()
        assert got == n and fail.cpu().tolist() == [M], (label, "body")
        if want is not None:
            assert np.array_equal(dev.out[: 6 * n].cpu().numpy(), want[True]), (label, "body")
        ok, back = gpu.decode_frame(d.t[GUARD: GUARD + d.n].cpu().numpy().reshape(-1, 9), gpu.DecoderContext(mode=1))
        if want is None:
            assert not ok and len(back) == 0, (label, "host")
        else:
            assert ok and np.array_equal(np.asarray(back).view(np.uint8).reshape(-1), want[True]), (label, "host")


# ---- d. batches -------------------------------------------------------------------------------------------------------------------------
BGUARD = tf.GUARD                                                       # 4096: the layout tf.split_out checks


def batch_to_dev(frames, stride):
    """The frames at `stride` behind BGUARD bytes, frame 0 at a 256-byte boundary, every other byte 0xFF -> (device tensor, address of frame 0)"""
    import torch
    buf = np.full(2 * BGUARD + len(frames) * stride, HIGH, np.uint8)
    for f, b in enumerate(frames):
        buf[BGUARD + f * stride: BGUARD + f * stride + len(b)] = b
    t = torch.from_numpy(buf).cuda()
    assert (t.data_ptr() + BGUARD) % 256 == 0
    return t, t.data_ptr() + BGUARD


def lift_rule(f):
    return "dense" if f % 2 == 1 else "sparse" if f % 3 == 0 else None


def batch_streams(orc, L, coded, t, seed0=77):
    """Per frame 0..t symbol errors per block built on the host, then the lifting of lift_rule(f) -> (unlifted, lifted) flat streams.
    `sparse` lifts the blocks m % 64 == 17 of a band; a band with fewer than 18 blocks takes m % 4 == 1 instead."""
    every, first = (64, 17) if min(int(L.band_blocks[b]) for b in range(9)) > 17 else (4, 1)
    plain, up = [], []
    for f, c in enumerate(coded):
        s = orc.inject_errors(np.asarray(c).reshape(-1, 9), int(L.header_syms), int(L.body_syms) // 26, seed0 + f, t)
        rule = lift_rule(f)
        u = s if rule is None else rp.lift(s, L, None, rule, seed0 + f, "batch", every, first)
        assert (rule is None) == (not (u > 26).any()) and np.array_equal(u % 27, s)
        plain.append(s.reshape(-1)); up.append(u.reshape(-1))
    return plain, up


def run_frames(gpu, frames, n_raw, fmt, cfg, extra=272):
    """decode_frames_async on the batch -> (plan, per-frame output bytes, verdict words); output gaps and guards checked by split_out"""
    import torch
    n = len(frames); n_in = len(frames[0]) // 9
    p = gpu.frames_plan(True, n_raw if fmt == gpu.FRAMES_WORDS else 2 * n_raw, n, cfg, fmt)
    ins, outs = tf.r16(9 * n_in) + extra, p.out_stride_min + 48
    d_in, a_in = batch_to_dev(frames, ins)
    d_out, a_out = tf.dev_out(n, outs)
    ver = torch.full((2 * n,), 7, dtype=torch.int32, device="cuda")
    gpu.decode_frames_async(a_in, n_in, ins, n, cfg, n_raw, a_out, outs, fmt, ver.data_ptr(), tf.stream())
    torch.cuda.synchronize()
    return p, tf.split_out(d_out, n, outs, p.out_bytes), ver.cpu().numpy().tolist()


@pytest.mark.parametrize("shape", [(3, 4861), (5, 100), (1000, 334)])
def test_batches(gpu, orc, shape):
    """t3hip_decode_frames_async, RS(26,20), pixels, RGB and raw words: odd frames lifted `dense`, every third `sparse`, the rest not, on
    0..3 errors per block.  Every frame is the oracle's decode of its own stream; a frame that is not lifted comes out byte for byte as
    in a run of the batch with no frame lifted; gaps and guards hold their fill."""
    n, n_px = shape
    px, coded = tf.oracle_batch(n, n_px, 1)
    cfg = gpu.make_cfg(mode=1, **tf.K20); n_raw = (n_px + 1) // 2; L = gpu.plan(n_raw, cfg)
    plain, up = batch_streams(orc, L, coded, 3)
    assert sum((u > 26).any() for u in up) >= n // 2
    want = []
    for f in range(n):
        rc, opx = orc.decode_frame(up[f].reshape(-1, 9), ol.make_cfg(mode=1, **tf.K20))
        assert rc == 0 and len(opx) == 2 * n_raw and np.array_equal(opx[:n_px], px[f]), f
        want.append({gpu.FRAMES_PIXELS: opx.view(np.uint8), gpu.FRAMES_RGB: orc.quant_to_rgb(opx), gpu.FRAMES_WORDS: np.asarray(orc.pack_pixels(opx)).reshape(-1)})
    for fmt in (gpu.FRAMES_PIXELS, gpu.FRAMES_RGB, gpu.FRAMES_WORDS):
        p, got, ver = run_frames(gpu, up, n_raw, fmt, cfg)
        assert p.one_launch == (0 if fmt == gpu.FRAMES_WORDS else 1)
        assert ver == [0] * (2 * n), (fmt, [i for i, v in enumerate(ver) if v][:10])
        _, base, bver = run_frames(gpu, plain, n_raw, fmt, cfg)
        assert bver == ver
        for f in range(n):
            assert np.array_equal(got[f], want[f][fmt]), "format %d: frame %d (%s) differs from the oracle's decode" % (fmt, f, lift_rule(f))
            if lift_rule(f) is None:
                assert np.array_equal(got[f], base[f]), "format %d: frame %d changed with its neighbours' bytes" % (fmt, f)


def test_batch_window(gpu, orc):
    """t3hip_decode_frames_window_async, 3 frames of 100 x 70, one window that starts in tile 1: the oracle's decode, cropped."""
    import torch
    from test_gpu_window import crop_np
    n, n_px, win = 3, 7000, (100, 70, 10, 22, 50, 20)
    px, coded = tf.oracle_batch(n, n_px, 1)
    cfg = gpu.make_cfg(mode=1, **tf.K20); n_raw = n_px // 2; L = gpu.plan(n_raw, cfg)
    _, up = batch_streams(orc, L, coded, 3)
    nb = win[4] * win[5] * 6; outs = tf.r16(nb) + 32
    assert gpu.frames_window_plan(n_raw, n, cfg, *win, gpu.WINDOW_PIXELS).one_launch == 1
    ins = tf.r16(len(up[0])) + 272
    d_in, a_in = batch_to_dev(up, ins)
    d_out, a_out = tf.dev_out(n, outs)
    ver = torch.full((2 * n,), 7, dtype=torch.int32, device="cuda")
    gpu.decode_frames_window_async(a_in, len(up[0]) // 9, ins, n, cfg, n_raw, *win, a_out, outs, gpu.WINDOW_PIXELS, ver.data_ptr(), tf.stream())
    torch.cuda.synchronize()
    got = tf.split_out(d_out, n, outs, nb)
    assert ver.cpu().tolist() == [0] * (2 * n)
    for f in range(n):
        rc, opx = orc.decode_frame(up[f].reshape(-1, 9), ol.make_cfg(mode=1, **tf.K20)); assert rc == 0
        assert np.array_equal(got[f], crop_np(opx, *win).view(np.uint8)), f


def test_batch_images(gpu, orc):
    """t3hip_decode_images_async, two 854 x 480 frames (frame 0 `sparse`, frame 1 `dense`): the oracle's decode through its RGB bridge."""
    import torch
    n, sub = 2, 15
    fw, fh, _, _, tw, th = gpu.image_geometry(sub, False)
    assert (fw, fh) == (tw, th) == (854, 480)
    px, coded = tf.oracle_batch(n, fw * fh, 1, 2, 3)
    cfg = gpu.make_cfg(mode=1, **tf.K20); n_raw = fw * fh // 2; L = gpu.plan(n_raw, cfg)
    _, up = batch_streams(orc, L, coded, 3)
    nb = tw * th * 3; outs = tf.r16(nb) + 32
    ins = tf.r16(len(up[0])) + 272
    d_in, a_in = batch_to_dev(up, ins)
    d_out, a_out = tf.dev_out(n, outs)
    ver = torch.full((2 * n,), 7, dtype=torch.int32, device="cuda")
    gpu.decode_images_async(a_in, len(up[0]) // 9, ins, n, cfg, sub, False, a_out, outs, ver.data_ptr(), tf.stream())
    torch.cuda.synchronize()
    got = tf.split_out(d_out, n, outs, nb)
    assert ver.cpu().tolist() == [0] * (2 * n)
    for f in range(n):
        rc, opx = orc.decode_frame(up[f].reshape(-1, 9), ol.make_cfg(mode=1, **tf.K20)); assert rc == 0
        assert np.array_equal(opx, px[f]) and np.array_equal(got[f], orc.quant_to_rgb(opx)), f


# ---- e. the header ------------------------------------------------------------------------------------------------------------------------
def _no_mode(d):
    return {k: v for k, v in d.items() if k not in ("mode", "superframe_words")}


@pytest.mark.parametrize("name", sorted(rp.CONFIGS))
def test_header_bytes(gpu, orc, name):
    """One header byte lifted, all of them lifted (congruent mod 27): the entries that parse the header on the host answer as the oracle
    does -- same configuration, word count and pixels -- and the device's byte compare answers "differs" (d_verdict[0] = 1), for which
    include/t3hip.h names the remedy: t3hip_decode_profile_dev."""
    import torch
    fr = _frame(name, "small")
    dev = Dev(gpu, fr)
    want = fr.padded.view(np.uint8).reshape(-1)
    for i, hdr in enumerate(header_lifts(fr)):
        oseen = ol.make_cfg(mode=1)
        rc, opx = orc.decode_frame(hdr, oseen)
        assert rc == 0 and np.array_equal(opx, fr.padded)
        d = Guarded(hdr)
        rc, c, n_raw = gpu.read_header_dev(d.data_ptr(), d.numel() // 9, 1, dev.s)
        assert rc == 0 and n_raw == fr.n_raw and _no_mode(c.as_dict()) == _no_mode(oseen.as_dict()), (name, i, "read_header_dev")
        rc, got, out = dev.run_sync(d, True)
        assert rc == 0 and got == dev.n_px and np.array_equal(out, want), (name, i, "decode_profile_dev")
        dctx = gpu.DecoderContext(mode=1)
        ok, back = gpu.decode_frame(hdr, dctx)
        assert ok and np.array_equal(np.asarray(back).view(np.uint8).reshape(-1), want), (name, i, "host")
        assert dctx.cfg_last_seen.as_dict() == oseen.as_dict(), (name, i, "host")
        ver, _ = dev.run_async(d, True)
        assert ver[0] == 1, (name, i, "decode_frame_async", ver)
    ver, out = dev.run_async(Guarded(fr.clean), True)                      # (the same call on the canonical header: 0, and the pixels)
    assert ver == [0, 0] and np.array_equal(out, want)


def test_header_bytes_in_a_batch(gpu, orc):
    """Frame 2 of five with a lifted header: its header word alone is 1; every other frame's words are 0 and its pixels the oracle's."""
    n, n_px, j = 5, 100, 2
    px, coded = tf.oracle_batch(n, n_px, 1)
    cfg = gpu.make_cfg(mode=1, **tf.K20); n_raw = n_px // 2; L = gpu.plan(n_raw, cfg)
    hs = int(L.header_syms)
    for which in ("one", "all"):
        frames = [np.array(c) for c in coded]
        at = np.array([5]) if which == "one" else np.arange(hs)
        frames[j] = rp.lift_bytes(frames[j], at, 9, "batch header")
        if which == "one":
            frames[j][5] = coded[j][5] + 27 * int(rp.max_mult(coded[j][5]))
        assert (frames[j][:hs] > 26).any() and np.array_equal(frames[j] % 27, coded[j])
        p, got, ver = run_frames(gpu, frames, n_raw, gpu.FRAMES_PIXELS, cfg)
        assert p.one_launch == 1 and [ver[2 * f] for f in range(n)] == [1 if f == j else 0 for f in range(n)], (which, ver)
        assert all(ver[2 * f + 1] == 0 for f in range(n) if f != j), (which, ver)
        for f in range(n):
            if f != j:
                assert np.array_equal(got[f].view(ol.PIXEL_DT)[:n_px], px[f]), (which, f)


# ---- f. COMPAT ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", COMPAT_NAMES)
def test_compat_streams(gpu, orc, name):
    """COMPAT streams the reference's decoder accepts, 26 / 600 / 5000 body words, 0 / 1 / 5 corruptions, every byte lifted (header
    included), through decode_profile_to_raw and decode_frame: the oracle's code, words, configuration and pixels on the same bytes."""
    for nbw, corrupt, s, up in compat_streams(orc, name):
        dctx = gpu.DecoderContext(); oseen = ol.make_cfg()
        ok, out = gpu.decode_profile_to_raw(up, dctx)
        rc, want = orc.decode_profile(up, oseen)
        assert ok == (rc == 0), (name, nbw, corrupt)
        assert np.array_equal(out, want if rc == 0 else want[:0]), (name, nbw, corrupt)
        assert _no_mode(dctx.cfg_last_seen.as_dict()) == _no_mode(oseen.as_dict()), (name, nbw, corrupt)
        okp, pix = gpu.decode_frame(up, gpu.DecoderContext())
        assert okp == (rc == 0), (name, nbw, corrupt)
        if rc == 0:
            assert np.array_equal(pix, orc.unpack_words(want)), (name, nbw, corrupt)
        assert rc == 0 or corrupt, (name, nbw)
