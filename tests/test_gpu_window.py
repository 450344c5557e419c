"""GPU tests of the window decode (t3hip_decode_window_async) and the image front end (resize_rgb_nn, image compose, encode_image /
decode_image), byte for byte against the oracle: its full decode + a numpy crop (+ its quant_to_rgb), numpy restatements of
resize_rgb_nn (old/include/io_image.hpp:102-124, float64, the reference's expressions) and the oracle's blit_center_rgb."""
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as ol
from test_window_plan import STD_RES, build_image_demo, centered_window

pytestmark = pytest.mark.gpu

SINGLE = {"p1_k24": dict(profile=0, uep=0), "p2_k22": dict(profile=1, uep=1), "p3_k20": dict(profile=2, uep=2), "p4_k18": dict(profile=3, uep=3)}
WHOLE = {"p5_tile64_luma": dict(profile=4, uep="luma", tile=(64, 64)), "p2_luma": dict(profile=1, uep="luma"),
         "p5_tile64_uniform20": dict(profile=4, uep=2, tile=(64, 64)), "p2_beacon83": dict(profile=1, uep=1, beacon=(83, 2, 1))}
# (fw, fh, x0, y0, w, h) on a stream of 960 x 540 pixels
WINDOWS = [
    (960, 540, 320, 180, 320, 180),    # centred
    (960, 540, 0, 0, 64, 48),          # top-left
    (960, 540, 860, 490, 100, 50),     # bottom-right
    (960, 540, 481, 270, 1, 1),        # one pixel
    (960, 540, 0, 0, 960, 540),        # the full frame
    (960, 540, 333, 101, 77, 33),      # odd x0 and w: rows at 2-byte alignment, odd byte counts
    (960, 540, 1, 1, 3, 5),
    (960, 500, 10, 470, 50, 60),       # runs past fh (the stream has those pixels: zero all the same)
    (960, 600, 0, 520, 960, 60),       # runs past the stream
    (958, 541, 7, 530, 945, 11),       # fw * fh is not the pixel count; the last row is cut by the end of the stream
    (960, 540, 100, 700, 20, 20),      # wholly behind the stream
]


def crop_np(px, fw, fh, x0, y0, w, h):
    """Output pixel (x, y) = stream pixel (y0 + y) fw + x0 + x; a row >= fh or a pixel behind the stream is a zero record."""
    out = np.zeros((h, w), px.dtype)
    yy, xx = np.meshgrid(np.arange(h, dtype=np.int64), np.arange(w, dtype=np.int64), indexing="ij")
    s = (y0 + yy) * fw + x0 + xx
    ok = ((y0 + yy) < fh) & (s < len(px))
    out[ok] = px[s[ok]]
    return out.reshape(-1)


def resize_np(src, dw, dh):
    """resize_rgb_nn, io_image.hpp:102-124, literally (float64)."""
    sh, sw = src.shape[:2]
    if sw <= 0 or sh <= 0:
        return np.zeros((dh, dw, 3), np.uint8)
    sy = np.clip(((np.arange(dh) + 0.5) * np.float64(sh) / dh).astype(np.int64), 0, sh - 1)
    sx = np.clip(((np.arange(dw) + 0.5) * np.float64(sw) / dw).astype(np.int64), 0, sw - 1)
    return src[sy][:, sx]


def compose_np(orc, src, sub, centered):
    tw, th = STD_RES[sub]
    work = src if src.shape[:2] == (th, tw) else resize_np(src, tw, th)
    if centered and sub != 27:
        return orc.blit_center_rgb(work, tw, th, 7680, 4320).reshape(4320, 7680, 3), work
    return np.ascontiguousarray(work), work


def coded_frame(gpu, orc, kw, n_px, seed, max_err):
    """A FIXED frame of n_px LCG pixels, encoded on the device, with 0..max_err symbol errors per block; (device tensor, n_enc, cfg, layout)"""
    import torch
    s = torch.cuda.current_stream().cuda_stream
    px = orc.lcg_pixels(n_px, seed)
    d_px = torch.from_numpy(px.view(np.uint8)).cuda()
    cfg = gpu.make_cfg(mode=1, **kw)
    n_raw = n_px // 2; n_enc = gpu.encoded_words(n_raw, cfg)
    coded = torch.zeros(n_enc * 9 + 64, dtype=torch.uint8, device="cuda")
    assert gpu.encode_frame_dev(d_px.data_ptr(), n_px, cfg, coded.data_ptr(), n_enc, s) == n_enc
    L = gpu.plan(n_raw, cfg)
    if max_err:
        gpu.inject_errors_dev(coded.data_ptr(), L.header_syms, L.body_syms // 26, 20261016 + seed, max_err, s)
    torch.cuda.synchronize()
    return coded, n_enc, cfg, L


def window_of(gpu, coded, n_enc, cfg, n_raw, win, fmt, misalign=0):
    """-> (bytes of the window, verdict words); the output buffer starts `misalign` bytes behind a 256-byte boundary and is guarded"""
    import torch
    fw, fh, x0, y0, w, h = win
    nb = w * h * (6 if fmt == gpu.WINDOW_PIXELS else 3)
    buf = torch.full((nb + 512,), 0xA5, dtype=torch.uint8, device="cuda")
    ver = torch.full((2,), 7, dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    gpu.decode_window_async(coded.data_ptr(), n_enc, cfg, n_raw, fw, fh, x0, y0, w, h, buf.data_ptr() + 256 + misalign, fmt, ver.data_ptr(), s)
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[: 256 + misalign] == 0xA5).all() and (host[256 + misalign + nb:] == 0xA5).all(), "the crop wrote outside its window buffer"
    return host[256 + misalign: 256 + misalign + nb], ver.cpu().tolist()


@pytest.mark.parametrize("name", sorted(SINGLE))
def test_window_decode_tile_range(gpu, orc, name):
    """FIXED, one k: every window, both output formats, equals the oracle's full decode of the same (corrupted, correctable) stream
    cropped in numpy (and its quant_to_rgb); the plan is a tile range."""
    NPX = 960 * 540; n_raw = NPX // 2
    t = (26 - {0: 24, 1: 22, 2: 20, 3: 18}[SINGLE[name]["profile"]]) // 2
    for max_err in (0, t):
        coded, n_enc, cfg, L = coded_frame(gpu, orc, SINGLE[name], NPX, 31 + max_err, max_err)
        rc, px = orc.decode_frame(coded[: n_enc * 9].cpu().numpy(), ol.make_cfg(mode=1, **SINGLE[name]))
        assert rc == 0 and len(px) == NPX
        for i, win in enumerate(WINDOWS):
            p = gpu.window_plan(n_raw, cfg, *win)
            assert p.tile_range == 1
            want = crop_np(px, *win)
            got, ver = window_of(gpu, coded, n_enc, cfg, n_raw, win, gpu.WINDOW_PIXELS, misalign=4 * (i % 4))
            assert ver == [0, 0] and np.array_equal(got, want.view(np.uint8)), (name, max_err, win, "pixels")
            got, ver = window_of(gpu, coded, n_enc, cfg, n_raw, win, gpu.WINDOW_RGB, misalign=4 * ((i + 1) % 4))
            assert ver == [0, 0] and np.array_equal(got, orc.quant_to_rgb(want)), (name, max_err, win, "rgb")


def test_window_rgb_matches_bridge_kernel(gpu, orc):
    """RGB out is bit-identical to t3hip_quant_to_rgb_dev on the pixels the same window returns."""
    import torch
    NPX = 960 * 540; n_raw = NPX // 2
    coded, n_enc, cfg, L = coded_frame(gpu, orc, SINGLE["p3_k20"], NPX, 77, 3)
    s = torch.cuda.current_stream().cuda_stream
    for win in WINDOWS[:6]:
        px6, _ = window_of(gpu, coded, n_enc, cfg, n_raw, win, gpu.WINDOW_PIXELS)
        rgb, _ = window_of(gpu, coded, n_enc, cfg, n_raw, win, gpu.WINDOW_RGB)
        n = win[4] * win[5]
        d_px = torch.from_numpy(px6.copy()).cuda(); d_rgb = torch.zeros(3 * n + 16, dtype=torch.uint8, device="cuda")
        gpu.quant_to_rgb_dev(d_px.data_ptr(), n, d_rgb.data_ptr(), s)
        torch.cuda.synchronize()
        assert np.array_equal(rgb, d_rgb[: 3 * n].cpu().numpy()), win


def test_window_decode_8k(gpu, orc):
    """One 8K frame (P3, RS(26,20), 0..3 errors per block): the four centred windows and an odd one against the oracle's full decode."""
    fw, fh = 7680, 4320; NPX = fw * fh; n_raw = NPX // 2
    coded, n_enc, cfg, L = coded_frame(gpu, orc, SINGLE["p3_k20"], NPX, 4711, 3)
    rc, px = orc.decode_frame(coded[: n_enc * 9].cpu().numpy(), ol.make_cfg(mode=1, **SINGLE["p3_k20"]))
    assert rc == 0 and len(px) == NPX
    wins = [(fw, fh) + centered_window(sub) for sub in (24, 21, 18, 15)] + [(fw, fh, 4001, 4000, 2999, 400)]
    for win in wins:
        p = gpu.window_plan(n_raw, cfg, *win)
        assert p.tile_range == 1 and p.tile_hi - p.tile_lo < p.n_tiles
        want = crop_np(px, *win)
        got, ver = window_of(gpu, coded, n_enc, cfg, n_raw, win, gpu.WINDOW_PIXELS)
        assert ver == [0, 0] and np.array_equal(got, want.view(np.uint8)), (win, "pixels")
        got, ver = window_of(gpu, coded, n_enc, cfg, n_raw, win, gpu.WINDOW_RGB, misalign=8)
        assert ver == [0, 0] and np.array_equal(got, orc.quant_to_rgb(want)), (win, "rgb")


@pytest.mark.parametrize("name", sorted(WHOLE))
def test_window_decode_whole_frame_path(gpu, orc, name):
    """Per-band k, 2-D and beacon frames (FIXED) have no tile range: the same windows equal the same crop of what
    t3hip_decode_frame_async returns for that stream."""
    import torch
    NPX = 960 * 540; n_raw = NPX // 2
    coded, n_enc, cfg, L = coded_frame(gpu, orc, WHOLE[name], NPX, 91, 1)
    s = torch.cuda.current_stream().cuda_stream
    full = torch.zeros(NPX * 6 + 64, dtype=torch.uint8, device="cuda"); ver = torch.full((2,), 7, dtype=torch.int32, device="cuda")
    assert gpu.decode_frame_async(coded.data_ptr(), n_enc, cfg, n_raw, full.data_ptr(), NPX, ver.data_ptr(), True, s) == NPX
    torch.cuda.synchronize()
    assert ver.cpu().tolist() == [0, 0]
    px = full[: NPX * 6].cpu().numpy().view(ol.PIXEL_DT)
    assert np.array_equal(px, orc.lcg_pixels(NPX, 91))
    for i, win in enumerate(WINDOWS):
        assert gpu.window_plan(n_raw, cfg, *win).tile_range == 0
        want = crop_np(px, *win)
        got, v = window_of(gpu, coded, n_enc, cfg, n_raw, win, gpu.WINDOW_PIXELS, misalign=4 * (i % 4))
        assert v == [0, 0] and np.array_equal(got, want.view(np.uint8)), (name, win, "pixels")
        got, v = window_of(gpu, coded, n_enc, cfg, n_raw, win, gpu.WINDOW_RGB)
        assert v == [0, 0] and np.array_equal(got, orc.quant_to_rgb(want)), (name, win, "rgb")


def test_window_refusals(gpu, orc):
    import torch
    NPX = 960 * 540; n_raw = NPX // 2
    coded, n_enc, cfg, L = coded_frame(gpu, orc, SINGLE["p3_k20"], NPX, 3, 0)
    out = torch.full((4096,), 0xA5, dtype=torch.uint8, device="cuda"); ver = torch.full((2,), 7, dtype=torch.int32, device="cuda")
    for args, code in [((960, 540, 958, 0, 3, 1), gpu.E_ARG), ((0, 540, 0, 0, 0, 1), gpu.E_ARG)]:
        with pytest.raises(gpu.T3Error) as e:
            gpu.decode_window_async(coded.data_ptr(), n_enc, cfg, n_raw, *args, out.data_ptr(), gpu.WINDOW_RGB, ver.data_ptr())
        assert e.value.code == code
    with pytest.raises(gpu.T3Error) as e:                                                                   # destination not 4-byte aligned
        gpu.decode_window_async(coded.data_ptr(), n_enc, cfg, n_raw, 960, 540, 0, 0, 4, 4, out.data_ptr() + 2, gpu.WINDOW_RGB, ver.data_ptr())
    assert e.value.code == gpu.E_ARG
    with pytest.raises(gpu.T3Error) as e:
        gpu.decode_window_async(coded.data_ptr(), n_enc, gpu.make_cfg(profile=gpu.ProfileID.RAW_MODE, mode=1), n_raw, 960, 540, 0, 0, 4, 4, out.data_ptr(), 1, ver.data_ptr())
    assert e.value.code == gpu.E_ARG
    with pytest.raises(gpu.T3Error) as e:                                                                   # a truncated stream
        gpu.decode_window_async(coded.data_ptr(), n_enc - 5, cfg, n_raw, 960, 540, 0, 0, 4, 4, out.data_ptr(), 1, ver.data_ptr())
    assert e.value.code == gpu.E_HEADER
    for (w, h) in [(0, 9), (9, 0), (0, 0)]:                                                                   # empty: nothing launched
        gpu.decode_window_async(coded.data_ptr(), n_enc, cfg, n_raw, 960, 540, 5, 5, w, h, out.data_ptr(), 1, ver.data_ptr())
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0xA5).all() and ver.cpu().tolist() == [7, 7]
    # another configuration's header: verdict[0]
    other = gpu.make_cfg(mode=1, profile=2, uep=2, seed=(1, 1, 2))
    gpu.decode_window_async(coded.data_ptr(), n_enc, other, n_raw, 960, 540, 0, 300, 10, 10, out.data_ptr(), 1, ver.data_ptr())   # (600 bytes of window)
    torch.cuda.synchronize()
    assert ver.cpu().tolist()[0] == 1


def test_window_isolation(gpu, orc):
    """A block that cannot be corrected spoils the windows of its own tile only.  Band 0's first block (coded symbols header_syms ..
    header_syms + 25; pixel tile t holds blocks [52 t, 52 t + 52) of every band, so this is tile 0) is overwritten on the host."""
    import torch
    NPX = 960 * 540; n_raw = NPX // 2; kw = SINGLE["p3_k20"]
    coded, n_enc, cfg, L = coded_frame(gpu, orc, kw, NPX, 17, 0)
    ocfg = ol.make_cfg(mode=1, **kw)
    clean = coded[: n_enc * 9].cpu().numpy()
    rc, px = orc.decode_frame(clean, ocfg)
    assert rc == 0 and np.array_equal(px, orc.lcg_pixels(NPX, 17))
    hs = int(L.header_syms)
    bad = None
    for seed in range(32):          # a random word lies within t = 3 of some RS(26,20) codeword about one time in eight: take the first seed that does not
        cand = clean.copy(); cand[hs: hs + 26] = np.random.default_rng(seed).integers(0, 27, 26, dtype=np.uint8)
        if orc.decode_frame(cand, ocfg)[0] != 0:
            bad = cand; break
    assert bad is not None, "no seed gave an uncorrectable block"
    restored = bad.copy(); restored[hs: hs + 26] = clean[hs: hs + 26]
    assert orc.decode_frame(restored, ocfg)[0] == 0                                    # the input condition: that block alone fails
    coded[: n_enc * 9] = torch.from_numpy(bad).cuda()
    s = torch.cuda.current_stream().cuda_stream
    full = torch.zeros(NPX * 6 + 64, dtype=torch.uint8, device="cuda"); ver = torch.full((2,), 7, dtype=torch.int32, device="cuda")
    gpu.decode_frame_async(coded.data_ptr(), n_enc, cfg, n_raw, full.data_ptr(), NPX, ver.data_ptr(), True, s)
    torch.cuda.synchronize()
    v = ver.cpu().tolist()
    assert v[0] == 0 and v[1] >= 1
    for win in [(960, 540, 320, 180, 320, 180), (960, 540, 0, 3, 960, 537), (960, 540, 860, 490, 100, 50)]:
        assert gpu.window_plan(n_raw, cfg, *win).tile_lo > 0
        for fmt in (gpu.WINDOW_PIXELS, gpu.WINDOW_RGB):
            got, v = window_of(gpu, coded, n_enc, cfg, n_raw, win, fmt)
            want = crop_np(px, *win)
            assert v == [0, 0], (win, v)
            assert np.array_equal(got, want.view(np.uint8) if fmt == gpu.WINDOW_PIXELS else orc.quant_to_rgb(want)), win
    for win in [(960, 540, 0, 0, 64, 48), (960, 540, 0, 0, 960, 540), (960, 540, 959, 0, 1, 1)]:
        assert gpu.window_plan(n_raw, cfg, *win).tile_lo == 0
        got, v = window_of(gpu, coded, n_enc, cfg, n_raw, win, gpu.WINDOW_RGB)
        assert v[0] == 0 and v[1] >= 1, (win, v)


RESIZES = [(13, 7, 64, 48), (200, 100, 31, 17), (640, 360, 854, 480), (1000, 700, 333, 211), (1, 1, 5, 4), (97, 53, 97, 53), (3, 1000, 1000, 3),
           (854, 480, 7680, 4320), (7680, 4320, 854, 480)]


@pytest.mark.parametrize("sw,sh,dw,dh", RESIZES)
def test_resize_rgb_nn(gpu, orc, sw, sh, dw, dh):
    import torch
    src = orc.lcg_rgb(sw * sh, 100 + sw).reshape(sh, sw, 3)
    want = torch.from_numpy(np.ascontiguousarray(resize_np(src, dw, dh)).reshape(-1)).cuda()
    d_src = torch.from_numpy(src.reshape(-1)).cuda()
    for mis in (0, 4):
        dst = torch.full((dw * dh * 3 + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        gpu.resize_rgb_nn_dev(d_src.data_ptr(), sw, sh, dst.data_ptr() + mis, dw, dh, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert bool(torch.equal(dst[mis: mis + dw * dh * 3], want)), (sw, sh, dw, dh, mis)
        assert bool((dst[:mis] == 0xA5).all()) and bool((dst[mis + dw * dh * 3:] == 0xA5).all())
    if dw * dh <= 1 << 20:
        assert np.array_equal(gpu.resize_rgb_nn(src, sw, sh, dw, dh), resize_np(src, dw, dh))              # the host-buffer form


def test_resize_rgb_nn_edges(gpu):
    import torch
    dst = torch.full((5 * 4 * 3 + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    gpu.resize_rgb_nn_dev(0, 0, 7, dst.data_ptr(), 5, 4)                                                     # no source: the destination is zeroed
    torch.cuda.synchronize()
    assert bool((dst[:60] == 0).all()) and bool((dst[60:] == 0xA5).all())
    for args in [(65536, 1, 4, 4), (4, 4, 65536, 1)]:
        with pytest.raises(gpu.T3Error) as e:
            gpu.resize_rgb_nn_dev(dst.data_ptr(), args[0], args[1], dst.data_ptr(), args[2], args[3])
        assert e.value.code == gpu.E_ARG


@pytest.mark.parametrize("sub", [27, 24, 21, 18, 15])
@pytest.mark.parametrize("centered", [0, 1])
def test_image_compose(gpu, orc, sub, centered):
    """resize (when the size differs) + centring blit in one kernel against numpy's resize and the oracle's blit, three source sizes"""
    import torch
    tw, th = STD_RES[sub]
    fw, fh = gpu.image_geometry(sub, centered)[:2]
    for (sw, sh) in [(tw, th), (640, 360), (1001, 701)]:
        src = orc.lcg_rgb(sw * sh, sub + sw).reshape(sh, sw, 3)
        frame, _ = compose_np(orc, src, sub, centered)
        assert frame.shape == (fh, fw, 3)
        want = torch.from_numpy(np.ascontiguousarray(frame).reshape(-1)).cuda()
        d_src = torch.from_numpy(src.reshape(-1)).cuda()
        dst = torch.full((fw * fh * 3 + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        gpu.image_compose_dev(d_src.data_ptr() + 0, sw, sh, sub, centered, dst.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert bool(torch.equal(dst[: fw * fh * 3], want)), (sub, centered, sw, sh)
        assert bool((dst[fw * fh * 3:] == 0xA5).all())


@pytest.mark.parametrize("sub,centered", [(15, 0), (15, 1), (24, 1), (21, 0)])
def test_encode_image_decode_image(gpu, orc, sub, centered):
    """encode_image_dev = encode_rgb_dev of the composed frame, byte for byte; decode_image_async of it = the oracle's bridge round trip
    of the resized image."""
    import torch
    s = torch.cuda.current_stream().cuda_stream
    sw, sh = 731, 411
    src = orc.lcg_rgb(sw * sh, 9 + sub).reshape(sh, sw, 3)
    frame, work = compose_np(orc, src, sub, centered)
    fw, fh, x0, y0, tw, th = gpu.image_geometry(sub, centered)
    n_px = fw * fh; n_raw = n_px // 2
    cfg = gpu.make_cfg(mode=1, profile=2, uep=2)
    n_enc = gpu.encoded_words(n_raw, cfg)
    d_src = torch.from_numpy(src.reshape(-1)).cuda()
    a = torch.zeros(n_enc * 9 + 64, dtype=torch.uint8, device="cuda"); b = torch.zeros_like(a)
    assert gpu.encode_image_dev(d_src.data_ptr(), sw, sh, sub, centered, cfg, a.data_ptr(), n_enc, s) == n_enc
    d_frame = torch.from_numpy(np.ascontiguousarray(frame).reshape(-1)).cuda()
    assert gpu.encode_rgb_dev(d_frame.data_ptr(), n_px, cfg, b.data_ptr(), n_enc, s) == n_enc
    torch.cuda.synchronize()
    assert bool(torch.equal(a, b))
    rgb = torch.full((tw * th * 3 + 64,), 0xA5, dtype=torch.uint8, device="cuda"); ver = torch.full((2,), 7, dtype=torch.int32, device="cuda")
    gpu.decode_image_async(a.data_ptr(), n_enc, cfg, sub, centered, rgb.data_ptr(), ver.data_ptr(), s)
    torch.cuda.synchronize()
    want = orc.quant_to_rgb(orc.rgb_to_quant(np.ascontiguousarray(work).reshape(-1)))
    assert ver.cpu().tolist() == [0, 0]
    assert np.array_equal(rgb[: tw * th * 3].cpu().numpy(), want) and bool((rgb[tw * th * 3:] == 0xA5).all())


@pytest.mark.parametrize("centered", [0, 1])
def test_image_names_demo_on_device(gpu, orc, tmp_path, centered):
    """The reference names of include/ternary_codec_v6.hpp: resize_rgb_nn, image_to_words_subword (RAW words of the composed frame),
    words_to_image_subword (exact-size branch / centre-window branch)."""
    exe = build_image_demo(str(tmp_path))
    sub, sw, sh, dw, dh = 15, 300, 200, 77, 91
    src = orc.lcg_rgb(sw * sh, 5).reshape(sh, sw, 3)
    p = lambda n: os.path.join(str(tmp_path), n)
    src.tofile(p("in.rgb"))
    subprocess.run([exe, str(sub), str(centered), str(sw), str(sh), p("in.rgb"), str(dw), str(dh), p("resized"), p("words"), p("rgb")], check=True)
    assert np.array_equal(np.fromfile(p("resized"), np.uint8), resize_np(src, dw, dh).reshape(-1))
    frame, work = compose_np(orc, src, sub, centered)
    q = orc.rgb_to_quant(np.ascontiguousarray(frame).reshape(-1))
    assert np.array_equal(np.fromfile(p("words"), np.uint8).reshape(-1, 9), orc.pack_pixels(q))
    assert np.array_equal(np.fromfile(p("rgb"), np.uint8), orc.quant_to_rgb(orc.rgb_to_quant(np.ascontiguousarray(work).reshape(-1))))
