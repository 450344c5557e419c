"""GPU tests of the window decode with erasures (include/t3hip.h, "decode a window with erasures"): decode_era_window_px<R, RGB, BCN>
(path 1: the window written straight from the tiles) and the private copy + erasure repair + window decode (path 0), against
expected_erasures of tests/erasure_patterns.py and the numpy crop of tests/test_gpu_window.py.  Frames: rs_patterns' "padded" (one-k:
at least 66 tiles, an odd pixel count, zero-padded last blocks) and "small" (301 pixels, below one tile) -- the smallest shapes where a
tile range, a ragged last tile and a frame smaller than a tile all occur.  The input sits in a guarded buffer that NO byte of may change
(tests/bounds.py), the output in a guarded buffer of exactly w * h * (6 | 3) bytes.  Byte work: every comparison is exact."""
import json
import os
import subprocess

import numpy as np
import pytest

import bounds
import erasure_patterns as ep
import oracle_lib as ol
import rs_patterns as rp
import test_gpu_decode_erasures as whole
from test_decode_erasures_plan import FUSED
from test_gpu_window import crop_np

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIXELS, RGB = 1, 2
SIZE = {PIXELS: 6, RGB: 3}
_frame, want_bytes = whole._frame, whole.want_bytes


def windows_of(N, k):
    """(fw, fh, x0, y0, w, h) for a stream of N pixels of a frame with tiles of 108 k pixels, by label.  fw = 251: prime, so the
    12-pixel groups straddle row ends and rows start at every alignment; fw = 108 k: rows are tile-aligned."""
    fw = 251; fh = -(-N // fw); T = 108 * k
    rem = N - (fh - 1) * fw                                                  # pixels of the stream's last row
    r1 = -(-T // fw) if N >= 2 * T else 0                                    # the first row that lies wholly in tile 1
    x_cut = max(min(rem, fw - 1) - 20, 0)
    out = {
        "full frame": (fw, fh, 0, 0, fw, fh),
        "one pixel": (fw, fh, 123, fh // 2, 1, 1),
        "top-left": (fw, fh, 0, 0, 64, min(48, fh)),
        "inside one tile": (fw, fh, 40, r1, 50, min(3, fh)),
        "bottom-right, cut by the stream's end": (fw, fh, x_cut, max(fh - 4, 0), min(60, fw - x_cut), min(4, fh)),
        "odd x0 and w": (fw, fh, 33, fh // 3, 77, min(33, fh)),
        "3 x 5": (fw, fh, 1, 1, 3, 5),
        "x0 + w == fw": (fw, fh, fw - 31, min(2, fh - 1), 31, min(7, fh)),
        "fw = 7": (7, -(-N // 7), 1, (N // 7) // 2, 5, 40),
        "past fh": (fw, max(fh - 3, 1), 10, max(fh - 10, 0), 50, 12),
        "past the stream": (fw, fh + 6, 0, max(fh - 2, 0), fw, 6),
        "behind the stream": (fw, fh + 40, 100, fh + 5, 20, 20),
    }
    fw2 = T; fh2 = -(-N // fw2)
    out["tile rows"] = (fw2, fh2, 0, min(1, fh2 - 1), fw2, min(3, fh2))
    out["tile rows, aligned groups"] = (fw2, fh2, 12, min(2, fh2 - 1), 36, min(4, fh2))
    out["tile rows, odd"] = (fw2, fh2, 13, fh2 // 2, 25, min(5, fh2))
    return out


def flagged_rows(fr, s):
    """bool per block, band after band: the block holds a byte above 26"""
    return (np.asarray(s)[rp.block_index(fr.L, fr.ocfg)] > 26).any(axis=1)


def decoded_blocks(fr, p):
    """bool per block, band after band: the call decodes it -- blocks 52 tile_lo <= m < 52 tile_hi of every band on a tile range of a
    path-1 plan, else every block"""
    f0 = rp.band_first_block(fr.L)
    m = np.concatenate([np.arange(n) for n in fr.blocks])
    assert len(m) == f0[8] + fr.blocks[8]
    if p.path == 1 and p.win.tile_range:
        return (m >= 52 * p.win.tile_lo) & (m < 52 * p.win.tile_hi)
    return np.ones(len(m), bool)


def words_among(fr, s, far, p):
    """[0, refused, flagged, flagged and accepted] among the blocks plan p decodes, from the yardstick's refused blocks `far`"""
    f0 = rp.band_first_block(fr.L)
    dec = decoded_blocks(fr, p); hi = flagged_rows(fr, s)
    refused = np.zeros(len(dec), bool)
    refused[np.array([f0[b] + m for b, m in far], np.int64)] = True
    return [0, int((refused & dec).sum()), int((hi & dec).sum()), int((hi & dec & ~refused).sum())]


class Call:
    """The input in one guarded buffer for a run of calls; every call's output in a guarded buffer of its own."""

    def __init__(self, gpu, fr, stream, offset=0, fill=bounds.FILLS[0]):
        b = np.ascontiguousarray(stream, np.uint8).reshape(-1)
        self.gpu, self.fr, self.fill, self.n_in = gpu, fr, fill, len(b) // 9
        self.inb = bounds.Buf(len(b), fill, offset, data=b, name="coded frame")       # no may_change range: read-only
        self.cfg = gpu.make_cfg(mode=1, **fr.kw)

    def window(self, win, fmt):
        """-> (the window's bytes, the four words)"""
        import torch
        out = bounds.Buf(win[4] * win[5] * SIZE[fmt], self.fill, 0, name="window")
        ver = torch.full((8,), 7, dtype=torch.int32, device="cuda")
        self.gpu.decode_erasures_window_async(self.inb.ptr, self.n_in, self.cfg, self.fr.n_raw, *win, out.ptr, fmt, ver.data_ptr(), torch.cuda.current_stream().cuda_stream)
        bounds.sync()
        v = ver.cpu().tolist()
        assert v[4:] == [7] * 4, ("words behind the verdict were written", v)
        return out.result(), v[:4]

    def done(self):
        self.inb.result()                                                    # the input byte-identical, its guards intact


# ---- 1. the recoverable sweep ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ("small", "padded"))
@pytest.mark.parametrize("name", sorted(rp.CONFIGS))
def test_recoverable_sweep(gpu, orc, name, what):
    """Every framing at two sizes, every admissible (s, e) in every band, nothing beyond capacity: every window in both formats is the
    numpy crop of the frame's own pixels, the words [0, 0, flagged, flagged] among the decoded blocks; the input is untouched at base
    offsets 0 and 2 mod 16, the output's guards intact under both fills."""
    fr = _frame(name, what)
    s, flagged = whole._recoverable(name, what)
    cfg = gpu.make_cfg(mode=1, **fr.kw)
    N = len(fr.padded)
    wins = windows_of(N, max(fr.ks))
    plans = {(lab, fmt): gpu.decode_erasures_window_plan(fr.n_raw, cfg, *win, fmt) for lab, win in wins.items() for fmt in (PIXELS, RGB)}
    want4 = {key: words_among(fr, s, [], p) for key, p in plans.items()}
    for key, p in plans.items():
        assert p.path == (1 if name in FUSED else 0), (name, key)
        if not (p.path == 1 and p.win.tile_range):
            assert want4[key] == [0, 0, flagged, flagged], (name, key)
    if name in rp.ONE_K and what == "padded":                                # the range is seen to matter, before any GPU call
        assert any(0 < w[2] < flagged for w in want4.values()), name
        assert want4[("behind the stream", PIXELS)] == [0, 0, 0, 0] and want4[("full frame", PIXELS)] == [0, 0, flagged, flagged]
    for fmt in (PIXELS, RGB):
        for offset, fill in ((0, bounds.FILLS[0]), (2, bounds.FILLS[1])):
            call = Call(gpu, fr, s, offset, fill)
            for lab, win in wins.items():
                got, ver = call.window(win, fmt)
                tag = (name, what, lab, win, fmt, offset)
                assert ver == want4[(lab, fmt)], (tag, ver, want4[(lab, fmt)])
                bounds.check_equal(got, want_bytes(orc, crop_np(fr.padded, *win), fmt), fill, "window %s" % (tag,))
            call.done()


# ---- 2. tile independence ---------------------------------------------------------------------------------------------------------------------
def good_run(n_tiles, bad):
    """the longest run [lo, hi) of tiles without a refused block"""
    best = (0, 0); lo = None
    for t in range(n_tiles + 1):
        if t < n_tiles and t not in bad:
            lo = t if lo is None else lo
        elif lo is not None:
            best = max(best, (lo, t), key=lambda r: r[1] - r[0]); lo = None
    return best


@pytest.mark.parametrize("name", rp.ONE_K)
def test_tile_independence(gpu, orc, name):
    """The full damage plan, beyond-capacity blocks included, and a window whose tiles hold no refused block while others do: word [1] is
    0, words [2] = [3] the flagged blocks of the decoded tiles, and the window is the crop of what the yardstick's stream decodes to."""
    fr = _frame(name, "padded")
    s, words, far, px = whole._beyond(name)
    k = fr.ks[0]; T = 108 * k; N = len(fr.padded); fw = 251; fh = -(-N // fw)
    n_tiles = -(-max(fr.blocks) // 52)
    bad = set(rp.far_tiles_one_k(k, far))
    lo, hi = good_run(n_tiles, bad)
    y0 = -(-lo * T // fw); y1 = min(hi * T, N) // fw                        # rows that lie wholly inside the run
    assert hi > lo and y1 > y0, (name, lo, hi)
    win = (fw, fh, 0, y0, fw, y1 - y0)
    cfg = gpu.make_cfg(mode=1, **fr.kw)
    call = Call(gpu, fr, s)
    for fmt in (PIXELS, RGB):
        p = gpu.decode_erasures_window_plan(fr.n_raw, cfg, *win, fmt)
        assert p.path == 1 and p.win.tile_range == 1 and lo <= p.win.tile_lo < p.win.tile_hi <= hi, (name, lo, hi, p.win.tile_lo, p.win.tile_hi)
        assert not any(p.win.tile_lo <= t < p.win.tile_hi for t in bad) and len(bad) > 0 and words[1] > 0      # refused blocks: outside only
        want4 = words_among(fr, s, far, p)
        assert want4[1] == 0 and want4[2] == want4[3] and 0 < want4[2] < words[4], (name, want4, words)
        got, ver = call.window(win, fmt)
        assert ver == want4, (name, fmt, ver, want4)
        bounds.check_equal(got, want_bytes(orc, crop_np(px, *win), fmt), call.fill, "window of good tiles, %s fmt %d" % (name, fmt))
    call.done()


# ---- 3. beyond capacity inside the window -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FUSED)
def test_beyond_capacity_inside_the_window(gpu, orc, name):
    """The same stream and windows that cover refused tiles -- the whole frame, and (one k without beacon) a range that ends inside it:
    the words are the yardstick's counts among the decoded blocks, every window byte whose stream pixel lies outside the refused tiles is
    the crop of what the yardstick's stream decodes to, and the synchronous entry returns T3_E_RS with the same counts."""
    import torch
    fr = _frame(name, "padded")
    s, words, far, px = whole._beyond(name)
    k = fr.ks[0]; N = len(fr.padded); fw = 251; fh = -(-N // fw)
    keep_px = rp.pixels_outside_tiles(N, k, rp.far_tiles_one_k(k, far))
    cfg = gpu.make_cfg(mode=1, **fr.kw)
    wins = [(fw, fh, 0, 0, fw, fh), (fw, fh, 7, fh // 5, 201, fh // 2)]
    checks = []
    for win in wins:                                                         # the conditions, before anything runs on the GPU
        p = gpu.decode_erasures_window_plan(fr.n_raw, cfg, *win, PIXELS)
        want4 = words_among(fr, s, far, p)
        in_stream = crop_np(np.ones(N, bool), *win)
        keep = crop_np(keep_px, *win) | ~in_stream                           # positions outside the stream are zero records: compared
        assert p.path == 1 and want4[1] > 0 and (keep & in_stream).sum() >= in_stream.sum() / 4, (name, win, want4)
        checks.append((win, want4, keep))
    assert checks[0][1] == [0, words[1], words[4], words[5]], (name, checks[0][1], words)
    if name in rp.ONE_K:
        assert checks[1][1][2] < words[4], name                             # the second window: a true range
    call = Call(gpu, fr, s)
    for win, want4, keep in checks:
        for fmt in (PIXELS, RGB):
            got, ver = call.window(win, fmt)
            assert ver == want4, (name, win, fmt, ver, want4)
            kb = np.repeat(keep, SIZE[fmt])
            assert np.array_equal(got[kb], want_bytes(orc, crop_np(px, *win), fmt)[kb]), (name, win, fmt)
    call.done()
    win, want4, keep = checks[1]
    b = np.ascontiguousarray(s, np.uint8).reshape(-1)
    inb = bounds.Buf(len(b), call.fill, 0, data=b, name="coded frame"); out = bounds.Buf(win[4] * win[5] * 6, call.fill, 0, name="window")
    seen = gpu.DecoderContext(mode=1).cfg_last_seen
    rc, counts = gpu.decode_erasures_window_dev(inb.ptr, len(b) // 9, seen, *win, out.ptr, PIXELS, torch.cuda.current_stream().cuda_stream)
    bounds.sync()
    assert rc == gpu.E_RS and counts == want4, (name, rc, counts, want4)
    inb.result()
    kb = np.repeat(keep, 6)
    assert np.array_equal(out.result()[kb], want_bytes(orc, crop_np(px, *win), PIXELS)[kb]), name


# ---- 4. equivalence to the whole-frame entry ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FUSED)
def test_equals_the_crop_of_the_whole_frame_entry(gpu, orc, name):
    """The recoverable stream: the pixel window is the numpy crop of t3hip_decode_erasures_frame_async's output, the RGB window
    t3hip_quant_to_rgb_dev on the pixel window."""
    import torch
    fr = _frame(name, "padded")
    s, _ = whole._recoverable(name, "padded")
    full, _ = whole.run(gpu, fr, s, PIXELS)
    full = full.view(ol.PIXEL_DT)
    call = Call(gpu, fr, s)
    wins = windows_of(len(fr.padded), fr.ks[0])
    for lab in ("full frame", "odd x0 and w", "fw = 7", "past the stream", "tile rows, odd"):
        win = wins[lab]
        got, _ = call.window(win, PIXELS)
        assert np.array_equal(got, crop_np(full, *win).view(np.uint8)), (name, lab)
        rgb, _ = call.window(win, RGB)
        d = torch.from_numpy(got.copy()).cuda(); o = torch.zeros(len(got) // 2, dtype=torch.uint8, device="cuda")
        gpu.quant_to_rgb_dev(d.data_ptr(), len(got) // 6, o.data_ptr(), torch.cuda.current_stream().cuda_stream)
        bounds.sync()
        assert np.array_equal(rgb, o.cpu().numpy()), (name, lab)
    call.done()


# ---- 5. path 0 ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("luma", "2d_64x64_k20"))
def test_path_0(gpu, orc, name):
    """Per-band k and 2-D: the private copy, the erasure repair and the window entry on the copy.  Bytes (recoverable stream) against the
    crop of the whole-frame erasure entry's output, words (a stream with refused blocks too) against that entry's."""
    fr = _frame(name, "small")
    s, _ = whole._recoverable(name, "small")
    mixed = ep.damage_frame(orc, fr, 45)[0]
    cfg = gpu.make_cfg(mode=1, **fr.kw)
    wins = windows_of(len(fr.padded), max(fr.ks))
    for stream, exact in ((s, True), (mixed, False)):
        full, w4 = whole.run(gpu, fr, stream, PIXELS)
        assert exact or w4[1] > 0
        call = Call(gpu, fr, stream, 2)
        for lab in ("full frame", "3 x 5", "fw = 7", "past the stream"):
            win = wins[lab]
            for fmt in (PIXELS, RGB):
                assert gpu.decode_erasures_window_plan(fr.n_raw, cfg, *win, fmt).path == 0
                got, ver = call.window(win, fmt)
                assert ver == w4, (name, lab, fmt, ver, w4)
                if exact:
                    assert np.array_equal(got, want_bytes(orc, crop_np(full.view(ol.PIXEL_DT), *win), fmt)), (name, lab, fmt)
        call.done()


# ---- 6. the synchronous and host entries --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("k20", "four_codes"))
def test_synchronous_entries(gpu, orc, name):
    """One fused and one generic configuration: a damaged but decodable header decodes (counts[0] stays 0) and `seen` becomes the frame's
    configuration; a header damaged beyond t is T3_E_HEADER with the guarded output untouched; the host entry's download equals the
    device entry's bytes, and the caller's input is not written."""
    import torch
    fr = _frame(name, "small")
    ok_s, flagged = whole._recoverable(name, "small")
    st = torch.cuda.current_stream().cuda_stream
    want_cfg = gpu.make_cfg(mode=1, **fr.kw)
    win = (7, 44, 1, 2, 5, 42)                                              # 301 pixels as rows of 7: the last window row ends behind the stream
    cases = (("header+2", whole._damage_header(ok_s, 2), gpu.OK, [0, 0, flagged, flagged]), ("header+9", whole._damage_header(ok_s, 9), gpu.E_HEADER, [0, 0, 0, 0]))
    for label, s, want_rc, want4 in cases:
        for fmt in (PIXELS, RGB):
            tag = (name, label, fmt)
            inb = bounds.Buf(len(s), bounds.FILLS[0], 2, data=s, name="coded frame"); out = bounds.Buf(win[4] * win[5] * SIZE[fmt], bounds.FILLS[0], 0, name="window")
            seen = gpu.DecoderContext(mode=1).cfg_last_seen
            rc, counts = gpu.decode_erasures_window_dev(inb.ptr, len(s) // 9, seen, *win, out.ptr, fmt, st)
            bounds.sync()
            assert rc == want_rc and counts == want4, (tag, rc, counts, want4)
            inb.result()
            before = s.copy()
            hrc, got, hcounts = gpu.decode_erasures_window(s.reshape(-1, 9), gpu.DecoderContext(mode=1), *win, fmt)
            assert hrc == want_rc and hcounts == want4 and np.array_equal(s, before), (tag, "host", hrc, hcounts)
            if want_rc == gpu.E_HEADER:
                out.untouched()
                assert got is None, tag
            else:
                assert seen.profile == want_cfg.profile and list(seen.band_profile) == list(want_cfg.band_profile) and seen.mode == 1, tag
                dev = out.result()
                bounds.check_equal(dev, want_bytes(orc, crop_np(fr.padded, *win), fmt), bounds.FILLS[0], "window %s" % (tag,))
                assert np.array_equal(np.ascontiguousarray(got).view(np.uint8).reshape(-1), dev), (tag, "host")
    with pytest.raises(gpu.T3Error) as e:                                     # seen->mode must be FIXED on entry
        gpu.decode_erasures_window(np.asarray(ok_s).reshape(-1, 9), gpu.DecoderContext(mode=0), *win, PIXELS)
    assert e.value.code == gpu.E_ARG


# ---- 7. the C++ demo ------------------------------------------------------------------------------------------------------------------------------
def test_decode_window_erasures_demo(gpu, orc, tmp_path):
    """tests/cpp/decode_window_erasures_demo.cpp: a viewer's crop of a received frame through decode_window_erasures of
    include/ternary_codec_v6.hpp, built with g++ alone: the recoverable stream gives the crop of the frame's own pixels, a header
    damaged beyond t no pixels at all."""
    lib = os.path.join(ROOT, "ternary-image-codec_amd")
    exe = str(tmp_path / "decode_window_erasures_demo")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "decode_window_erasures_demo.cpp"),
                    "-L" + lib, "-lt3hip", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-o", exe], check=True)
    fr = _frame("k20", "small")
    s, flagged = whole._recoverable("k20", "small")
    win = (7, 44, 1, 2, 5, 42)
    fin, fout = str(tmp_path / "in.words"), str(tmp_path / "out.px")
    np.asarray(s).tofile(fin)
    out = json.loads(subprocess.run([exe, fin] + [str(x) for x in win] + [fout], check=True, capture_output=True, text=True).stdout)
    assert out == {"ok": 1, "status": 0, "pixels": 5 * 42, "counts": [0, flagged, flagged]}, out
    assert np.array_equal(np.fromfile(fout, np.uint8), crop_np(fr.padded, *win).view(np.uint8))
    whole._damage_header(s, 9).tofile(fin)
    out = json.loads(subprocess.run([exe, fin] + [str(x) for x in win] + [fout], check=True, capture_output=True, text=True).stdout)
    assert out == {"ok": 0, "status": gpu.E_HEADER, "pixels": 0, "counts": [0, 0, 0]}, out


# ---- 8. path 0 from a parsed header: the scrambler is the stream's, not the header's seeds mod 27 -----------------------------------------
WRAP_SEED = (0xFFFFFFFF, 0xFFFFFFFE, 5)                                     # a * s + b wraps 2^32: the next-state table differs from that of (21, 20, 5)


@pytest.mark.parametrize("name", ("four_codes", "2d_64x64_k20"))
def test_path_0_parsed_header_wrapping_seed(gpu, orc, name):
    """The synchronous and host entries on a path-0 configuration whose scrambler seeds wrap 2^32: the parsed header carries the seeds mod
    27 and the scrambler as its next-state table, and the window decode of the repaired copy must run on the table.  Windows against the
    crop of the frame's own pixels and of t3hip_decode_erasures_profile_dev's output on the same stream."""
    import torch
    cfg = gpu.make_cfg(mode=1, seed=WRAP_SEED, **rp.CONFIGS[name])
    fr = rp.make_frame(orc, lambda n_raw: gpu.plan(n_raw, cfg), name, "small", scr=WRAP_SEED)
    plain = _frame(name, "small")
    assert not np.array_equal(fr.clean, plain.clean) and np.array_equal(fr.px, plain.px)          # the seed reaches the wire, not the pixels
    s, _ = ep.damage_frame(orc, fr, whole.SEED["small"], only=ep.admissible(max(fr.ks)) + ["sched", "clean"])
    _, words, far = ep.expected_erasures(orc, fr, s)
    assert words[1] == 0 and far == [] and words[4] == words[5] > 0
    want4 = [0, 0, words[4], words[4]]
    st = torch.cuda.current_stream().cuda_stream
    inb = bounds.Buf(len(s), bounds.FILLS[0], 2, data=s, name="coded frame")
    full = bounds.Buf(12 * fr.n_raw, bounds.FILLS[0], 0, name="whole frame")
    rc, n, counts = gpu.decode_erasures_profile_dev(inb.ptr, len(s) // 9, gpu.DecoderContext(mode=1).cfg_last_seen, full.ptr, 2 * fr.n_raw, PIXELS, st)
    bounds.sync()
    assert rc == gpu.OK and n == 2 * fr.n_raw and counts == want4, (name, rc, counts, want4)
    whole_px = full.result().view(ol.PIXEL_DT)
    assert np.array_equal(whole_px, fr.padded), name
    wins = windows_of(len(fr.padded), max(fr.ks))
    for lab in ("full frame", "3 x 5", "fw = 7", "past the stream"):
        win = wins[lab]
        for fmt in (PIXELS, RGB):
            tag = (name, lab, fmt)
            assert gpu.decode_erasures_window_plan(fr.n_raw, cfg, *win, fmt).path == 0, tag
            out = bounds.Buf(win[4] * win[5] * SIZE[fmt], bounds.FILLS[0], 0, name="window")
            rc, counts = gpu.decode_erasures_window_dev(inb.ptr, len(s) // 9, gpu.DecoderContext(mode=1).cfg_last_seen, *win, out.ptr, fmt, st)
            bounds.sync()
            assert rc == gpu.OK and counts == want4, (tag, rc, counts, want4)
            want = want_bytes(orc, crop_np(whole_px, *win), fmt)
            out.expect(want)
            hrc, got, hcounts = gpu.decode_erasures_window(s.reshape(-1, 9), gpu.DecoderContext(mode=1), *win, fmt)
            assert hrc == gpu.OK and hcounts == want4 and np.array_equal(np.ascontiguousarray(got).view(np.uint8).reshape(-1), want), (tag, "host")
    inb.result()
