"""GPU tests of the window decode with erasures over a batch of equal frames (include/t3hip.h, "decode a window with erasures of a batch of
equal FIXED frames"): decode_era_frames_window_px<R, RGB, BCN> -- ONE launch over the window's tiles of all frames -- where the plan says
so, the loop of the single-frame window body elsewhere, and the synchronous entries.  The yardsticks are erasure_patterns.expected_erasures
(proven on the CPU in tests/test_erasure_semantics.py), the numpy crop of tests/test_gpu_window.py, and t3hip_decode_erasures_window_async
on each frame alone: what a batch gives for frame f -- window bytes and the four words -- is what that entry gives for it.

Frames: rs_patterns' "small" (301 pixels, below one tile), "padded" (at least 66 tiles, an odd pixel count) and the 7-tile ragged frame of
tests/test_gpu_decode_erasures_frames.py: the smallest shapes with a tile range, a ragged last tile and a frame below a tile.
Guarding (tests/bounds.py): the coded batch sits in a buffer with NO range that may change, so a written byte of a frame or of a stride
gap fails; the output sits in a buffer whose only ranges that may change are the frames' out_bytes spans; the verdict tensor holds two
spare words behind 4 N that must stay.  Byte work: every comparison is exact.

Where a frame holds refused blocks its window is compared outside the pixel tiles of those blocks only.  So that such a comparison cannot
pass on a window that is mostly masked, every compared (stream, window) pair masks at most half of the window's bytes and every batch holds
a frame compared in full: mask_conditions, asserted at run time here and, with the yardstick alone, for every such pair in
tests/test_decode_erasures_frames_window_plan.py (MASKED lists them)."""
import json
import os
import subprocess

import numpy as np
import pytest

import bounds
import erasure_patterns as ep
import rs_patterns as rp
import test_gpu_decode_erasures as whole
import test_gpu_decode_erasures_frames as eframes
from test_decode_erasures_plan import FUSED
from test_gpu_decode_erasures_window import PIXELS, RGB, SIZE, Call, windows_of, words_among
from test_gpu_erasure_frames import expected_of, layout, round16, stream_of
from test_gpu_window import crop_np

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = bounds.FILLS[0]
SPARE = 0x07070707                                                        # the two words behind the 4 N verdict words
_frame, want_bytes, far_of, four = whole._frame, whole.want_bytes, eframes.far_of, eframes.four
BEYOND = ("damaged", 44)                                                  # damage_frame's own plan, beyond-capacity pairs included, at its own spacing


# ---- the runner -------------------------------------------------------------------------------------------------------------------------
class Batch:
    """The coded frames in one guarded buffer for a run of calls; every call's output in a guarded buffer of its own, of which only the
    frames' out_bytes spans may change; two spare words behind the verdict."""

    def __init__(self, gpu, fr, frames, in_stride=None, offset=0, fill=FILL):
        self.gpu, self.fr, self.fill, self.M = gpu, fr, fill, len(frames)
        self.cfg = gpu.make_cfg(mode=1, **fr.kw)
        self.nb = len(frames[0])
        self.in_stride = self.nb + (self.nb & 1) if in_stride is None else in_stride
        data, _ = layout(frames, self.in_stride if self.M > 1 else self.nb)
        self.inb = bounds.Buf(len(data), fill, offset, data=data, name="coded batch")    # no may_change range: read-only, gaps included

    def plan(self, win, fmt, n_frames=None):
        p = self.gpu.decode_erasures_frames_window_plan(self.fr.n_raw, self.M if n_frames is None else n_frames, self.cfg, *win, fmt)
        ob = win[4] * win[5] * SIZE[fmt]
        assert p.frame.in_bytes == self.nb and p.in_stride_min == self.nb + (self.nb & 1) and p.out_bytes == ob and p.out_stride_min == round16(ob)
        return p

    def window(self, win, fmt, out_stride=None, n_frames=None):
        """One t3hip_decode_erasures_frames_window_async -> ([each frame's window bytes], [its four words], the plan)"""
        import torch
        N = self.M if n_frames is None else n_frames
        p = self.plan(win, fmt)
        ob = int(p.out_bytes)
        out_stride = int(p.out_stride_min) if out_stride is None else out_stride
        ostep = out_stride if self.M > 1 else ob
        spans = tuple((f * ostep, f * ostep + ob) for f in range(self.M))
        out = bounds.Buf(0, self.fill, 0, data=np.full(max(spans[-1][1], 16), self.fill, np.uint8), name="window batch", may_change=spans if N and ob else ())
        ver = torch.full((4 * self.M + 2,), SPARE, dtype=torch.int32, device="cuda")
        self.gpu.decode_erasures_frames_window_async(self.inb.ptr, self.nb // 9, self.in_stride, N, self.cfg, self.fr.n_raw, *win, out.ptr, out_stride, fmt, ver.data_ptr(),
                                                     torch.cuda.current_stream().cuda_stream)
        bounds.sync()
        got = out.result()                                                  # guards and gaps intact
        v = ver.cpu().tolist()
        done = N if ob else 0
        assert v[4 * done:] == [SPARE] * (len(v) - 4 * done), ("words behind the batch's verdict words were written", v)
        return [got[lo:hi] for lo, hi in spans], [v[4 * f: 4 * f + 4] for f in range(self.M)], p

    def done(self):
        self.inb.result()                                                   # the input byte-identical, gaps included, its guards intact


def keep_of(fr, far, win):
    """bool per window position: compared -- its stream pixel lies outside the pixel tiles of the refused blocks `far`, or it maps to no
    stream pixel (a zero record)"""
    N = len(fr.padded)
    in_stream = crop_np(np.ones(N, bool), *win)
    return crop_np(rp.pixels_outside_tiles(N, fr.ks[0], rp.far_tiles_one_k(fr.ks[0], far)), *win) | ~in_stream


def mask_conditions(fr, fars, win, tag):
    """The conditions under which 'equal outside refused tiles' says something: every frame's mask leaves out at most half of the window,
    and one frame of the batch is compared in full -> the masks (None: in full)"""
    keeps = [keep_of(fr, far, win) if far else None for far in fars]
    for f, k in enumerate(keeps):
        assert k is None or 2 * int((~k).sum()) <= k.size, (tag, "frame", f, "masked", int((~k).sum()), "of", k.size)
    assert any(k is None or k.all() for k in keeps), (tag, "no frame is compared in full")
    return keeps


def check_masked(got, want, keep, fmt, fill, tag):
    if keep is None:
        bounds.check_equal(got, want, fill, "window %s" % (tag,))
    else:
        kb = np.repeat(keep, SIZE[fmt])
        assert np.array_equal(got[kb], want[kb]), tag


# ---- 1. the batch sweep -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ("small", "padded"))
@pytest.mark.parametrize("name", sorted(rp.CONFIGS))
def test_batch_sweep(gpu, orc, name, what):
    """Every framing at two sizes, three frames (recoverable A, clean, recoverable B), every window label in both formats; base offset 0
    with the smallest strides and base offset 2 mod 16 with gaps in both strides, one fill each.  Every frame's window is the numpy crop
    of the frame's own pixels, its words are the yardstick's among the blocks the plan decodes, and the batch runs as planned."""
    fr = _frame(name, what)
    sA, flA = whole._recoverable(name, what)
    cB, flB = eframes.recoverable_b(orc, fr, what, flA)
    frames = [np.asarray(sA).reshape(-1), stream_of(orc, fr, "clean"), stream_of(orc, fr, cB)]
    assert flA != flB
    wins = windows_of(len(fr.padded), max(fr.ks))
    nb = len(frames[0])
    seen_loop = seen_one = False
    for offset, fill, in_stride, gap in ((0, bounds.FILLS[0], None, 0), (2, bounds.FILLS[1], round16(nb) + 32, 48)):
        batch = Batch(gpu, fr, frames, in_stride, offset, fill)
        for fmt in (PIXELS, RGB):
            for lab, win in wins.items():
                tag = (name, what, lab, win, fmt, offset)
                p = batch.plan(win, fmt)
                assert p.one_launch == (1 if name in FUSED and p.frame.tiles_launched > 0 else 0) and p.frame.path == (1 if name in FUSED else 0), tag
                seen_loop |= p.one_launch == 0; seen_one |= p.one_launch == 1
                got, ver, _ = batch.window(win, fmt, out_stride=int(p.out_stride_min) + gap)
                want = want_bytes(orc, crop_np(fr.padded, *win), fmt)
                for f, s in enumerate(frames):
                    want4 = words_among(fr, s, [], p.frame)
                    assert ver[f] == want4, (tag, f, ver[f], want4)
                    bounds.check_equal(got[f], want, fill, "window %s frame %d" % (tag, f))
        batch.done()
    # "behind the stream" loops on a tile range, every window on path 0; with a beacon every tile of every frame is launched
    assert seen_one == (name in FUSED) and seen_loop == (name not in FUSED or name in rp.ONE_K), (name, seen_one, seen_loop)


# ---- 2. against the single-frame entry ------------------------------------------------------------------------------------------------
def good_runs(n_tiles, bad):
    """every maximal run [lo, hi) of tiles outside `bad`"""
    out = []; lo = None
    for t in range(n_tiles + 1):
        if t < n_tiles and t not in bad:
            lo = t if lo is None else lo
        elif lo is not None:
            out.append((lo, t)); lo = None
    return out


def rows_of_a_good_run(fr, far, fw=251):
    """Rows of fw pixels around the longest run [lo, hi) of tiles without a refused block of `far` (tile 0 counted as refused: far1's)
    that a refused tile follows -> (y0, y_good, y_in): rows [y0, y_good) lie wholly inside the run, row y_in in the middle of tile hi"""
    k = fr.ks[0]; T = 108 * k
    n_tiles = -(-max(fr.blocks) // 52)
    bad = set(rp.far_tiles_one_k(k, far)) | {0}
    runs = [r for r in good_runs(n_tiles, bad) if r[1] < n_tiles]
    lo, hi = max(runs, key=lambda r: r[1] - r[0])
    y0, y_good, y_in = -(-lo * T // fw), hi * T // fw, (hi * T + T // 2) // fw
    assert hi > lo and y_good > y0 and y_in > y_good, (fr.name, lo, hi)
    return y0, y_good, y_in


def mixed_batch(orc, name):
    """-> (frame, the cases recoverable | beyond capacity | clean | far1, their refused blocks, the three windows: the whole frame, a
    range of rows that starts in good tiles and ends inside a refused tile of the beyond-capacity frame, rows of good tiles only)"""
    fr = eframes.keep_frame(_frame(name, "padded"))
    rec = ("damaged", whole.SEED["padded"], tuple(ep.admissible(max(fr.ks)) + ["sched", "clean"]))       # _recoverable's stream
    cases = [rec, BEYOND, "clean", "far1"]
    fars = [far_of(orc, fr, c) for c in cases]
    assert fars[0] == [] and fars[2] == [] and len(fars[1]) > 0 and rp.far_tiles_one_k(fr.ks[0], fars[3]) == [0]
    w = expected_of(orc, fr, BEYOND)[1]
    assert 0 < w[5] < w[4] and w[1] > 0, (name, w)
    fw = 251; fh = -(-len(fr.padded) // fw)
    y0, y_good, y_in = rows_of_a_good_run(fr, fars[1])
    return fr, cases, fars, {"whole frame": (fw, fh, 0, 0, fw, fh), "ends inside a refused tile": (fw, fh, 7, y0, 201, y_in - y0), "good tiles only": (fw, fh, 0, y0, fw, y_good - y0)}


@pytest.mark.parametrize("name", FUSED)
def test_against_the_single_frame_entry(gpu, orc, name):
    """Recoverable, beyond capacity, clean and far1 in one batch, three windows, both formats: every frame's four words are those of
    t3hip_decode_erasures_window_async on it alone (and the yardstick's among the decoded blocks), its bytes equal that entry's outside
    the refused tiles, and the clean frame is compared in full against the frame's own pixels."""
    fr, cases, fars, wins = mixed_batch(orc, name)
    frames = [stream_of(orc, fr, c) for c in cases]
    batch = Batch(gpu, fr, frames)
    alone = [Call(gpu, fr, s) for s in frames]
    refused_seen = 0
    for lab, win in wins.items():
        keeps = mask_conditions(fr, fars, win, (name, lab))
        for fmt in (PIXELS, RGB):
            got, ver, p = batch.window(win, fmt)
            assert p.one_launch == 1, (name, lab)
            for f, c in enumerate(cases):
                tag = (name, lab, fmt, f, c)
                one, one4 = alone[f].window(win, fmt)
                assert ver[f] == one4 == words_among(fr, frames[f], fars[f], p.frame), (tag, ver[f], one4)
                check_masked(got[f], one, keeps[f], fmt, FILL, tag)
                refused_seen += ver[f][1]
            bounds.check_equal(got[2], want_bytes(orc, crop_np(fr.padded, *win), fmt), FILL, "the clean frame %s" % ((name, lab, fmt),))
        if name in rp.ONE_K and lab != "whole frame":
            assert 0 < p.frame.tiles_launched < p.frame.win.n_tiles, (name, lab)                # a true range
    assert refused_seen > 0
    batch.done()
    for c in alone:
        c.done()


# ---- 3. addresses -----------------------------------------------------------------------------------------------------------------------
def address_batch(t3, orc, name):
    """-> (the odd-sized frame of test_gpu_decode_erasures_frames.py, its cases A | far1 | clean | B, their refused blocks, two windows of
    odd w: the whole frame and one whose tiles start behind tile 0)"""
    fr = eframes._small_odd(t3, orc, name)
    cases = eframes.address_cases(orc, fr)
    fars = [far_of(orc, fr, c) for c in cases]
    fw = 251; N = len(fr.padded); fh = -(-N // fw); T = 108 * fr.ks[0]
    y1 = -(-T // fw) + 1
    return fr, cases, fars, {"whole frame": (fw, fh, 0, 0, fw, fh), "behind tile 0": (fw, fh, 33, y1, 77, 5)}


@pytest.mark.parametrize("name", ("k20", "k20_beacon83"))
def test_addresses(gpu, orc, name):
    """Base at 2 mod 16 and frames of an odd byte count in_bytes + 1 apart: every frame but the first starts off every 4-byte boundary;
    w is odd, so out_bytes is no multiple of 16 and the output stride has a gap; one window's tiles start behind tile 0.  Both fills."""
    fr, cases, fars, wins = address_batch(gpu, orc, name)
    frames = [stream_of(orc, fr, c) for c in cases]
    nb = len(frames[0])
    assert nb % 2 == 1 and len({(2 + f * (nb + 1)) % 16 for f in range(len(cases))}) > 1
    for fill in bounds.FILLS:
        batch = Batch(gpu, fr, frames, nb + 1, 2, fill)
        for lab, win in wins.items():
            keeps = mask_conditions(fr, fars, win, (name, lab))
            p = batch.plan(win, PIXELS)
            assert p.out_bytes % 16 != 0 and p.one_launch == 1, (name, lab)
            if name == "k20" and lab == "behind tile 0":
                assert 0 < p.frame.win.tile_lo < p.frame.win.tile_hi, (name, lab)
            got, ver, _ = batch.window(win, PIXELS)
            for f, c in enumerate(cases):
                tag = (name, fill, lab, f, c)
                assert ver[f] == words_among(fr, frames[f], fars[f], p.frame), (tag, ver[f])
                check_masked(got[f], want_bytes(orc, crop_np(eframes._pixels(fr.name, fr.n_px, c), *win), PIXELS), keeps[f], PIXELS, fill, tag)
        batch.done()


# ---- 4. frame crossing ------------------------------------------------------------------------------------------------------------------
CROSS_WIN = (251, 57, 0, 18, 251, 25)                                      # rows 18 .. 42 of a 7-tile k = 20 frame: stream pixels 4518 .. 10792, tiles 2, 3, 4


def crossing_batch(t3, orc, name):
    """-> (the 7-tile ragged frame of test_gpu_decode_erasures_frames.py, the cycle of its crossing_cases, their refused blocks)"""
    cfg = t3.make_cfg(mode=1, **rp.CONFIGS[name])
    fr = eframes.keep_frame(rp.Frame(orc, lambda n_raw: t3.plan(n_raw, cfg), name, 7 * 2160 - 1001, 104))
    cycle = eframes.crossing_cases(orc, fr)
    assert -(-len(fr.padded) // 251) == CROSS_WIN[1]
    return fr, cycle, [far_of(orc, fr, c) for c in cycle]


def crossing_windows(name):
    return (CROSS_WIN,) + (((251, 57, 0, 0, 251, 57),) if name == "k20_beacon83" else ())


@pytest.mark.parametrize("name", ("k20", "k20_beacon83"))
def test_frame_crossing(gpu, orc, name):
    """Frames of 7 tiles, the last ragged and the pixel count odd; the window covers a proper sub-range of the tiles (one k: tiles 2 to 4
    are launched; with a beacon every tile is), and so many frames that every workgroup (two per CU) draws more than two tickets and
    changes frame off the grid's rhythm; four streams cycled over the frames.  Per-frame words are exact and so are the sums over the
    frames of words 1 to 3 -- a lost or doubled flush at a frame change and a wrong frame base show; bytes outside the refused tiles are
    exact.  The beacon configuration runs once more on the whole-frame window."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    fr, cycle, cfars = crossing_batch(gpu, orc, name)
    cfg = gpu.make_cfg(mode=1, **fr.kw)
    for win in crossing_windows(name):
        one = gpu.decode_erasures_window_plan(fr.n_raw, cfg, *win, PIXELS)
        if name == "k20":
            assert one.win.tile_range == 1 and 0 < one.win.tile_lo and one.win.tile_hi < 7 and one.win.n_tiles == 7, (one.win.tile_lo, one.win.tile_hi)
        per = one.tiles_launched
        assert per == (one.win.tile_hi - one.win.tile_lo if name == "k20" else 7)
        n_frames = -(-(9 * cus + 1) // per)
        cases = [cycle[f % 4] for f in range(n_frames)]
        keeps = dict(zip(cycle, mask_conditions(fr, cfars, win, (name, win))))
        batch = Batch(gpu, fr, [stream_of(orc, fr, c) for c in cases])
        got, ver, p = batch.window(win, PIXELS)
        batch.done()
        assert p.one_launch == 1 and p.tiles_launched == n_frames * per >= 9 * cus + 1
        want4 = {c: words_among(fr, stream_of(orc, fr, c), far, p.frame) for c, far in zip(cycle, cfars)}
        wrong = [(f, cases[f], ver[f], want4[cases[f]]) for f in range(n_frames) if ver[f] != want4[cases[f]]]
        assert not wrong, (len(wrong), wrong[:4])
        for i in (1, 2, 3):
            assert sum(v[i] for v in ver) == sum(want4[c][i] for c in cases), ("word", i)
        assert sum(v[2] for v in ver) > 0
        wants = {c: want_bytes(orc, crop_np(eframes._pixels(fr.name, fr.n_px, c), *win), PIXELS) for c in cycle}
        for f, c in enumerate(cases):
            check_masked(got[f], wants[c], keeps[c], PIXELS, FILL, (name, win, "frame", f, c))


# ---- 5. zero fill -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("k20", "k20_beacon83", "luma"))
def test_zero_fill(gpu, orc, name):
    """Windows past fh, past the stream's end and wholly behind the stream, three frames, an output stride with a gap: positions no pixel
    maps to are zero records, the gaps keep their fill (the guarded buffer), and "behind the stream" on a tile range takes the loop path
    with words [0, 0, 0, 0]."""
    fr = _frame(name, "padded")
    sA, flA = whole._recoverable(name, "padded")
    frames = [np.asarray(sA).reshape(-1), stream_of(orc, fr, "clean"), np.asarray(sA).reshape(-1)]
    wins = windows_of(len(fr.padded), max(fr.ks))
    batch = Batch(gpu, fr, frames)
    for lab in ("past fh", "past the stream", "behind the stream"):
        win = wins[lab]
        for fmt in (PIXELS, RGB):
            p = batch.plan(win, fmt)
            assert p.frame.zero_fill == 1, (name, lab)
            got, ver, _ = batch.window(win, fmt, out_stride=int(p.out_stride_min) + 64)
            want = want_bytes(orc, crop_np(fr.padded, *win), fmt)
            assert not crop_np(np.ones(len(fr.padded), bool), *win).all()
            for f, s in enumerate(frames):
                assert ver[f] == words_among(fr, s, [], p.frame), (name, lab, fmt, f, ver[f])
                bounds.check_equal(got[f], want, FILL, "zero-filled window %s" % ((name, lab, fmt, f),))
            if lab == "behind the stream":
                assert not want.any()
                if name == "k20":
                    assert p.one_launch == 0 and p.frame.path == 1 and p.frame.tiles_launched == 0 and ver == [[0, 0, 0, 0]] * 3, (name, ver)
    batch.done()


# ---- 6. the header word -----------------------------------------------------------------------------------------------------------------
def test_header_word(gpu, orc):
    """One header symbol of frame 1 of four changed; in another run a header byte of frame 2 set to 0xFF: only that frame's word 4 f is
    1, and every window is still the crop of the frame's pixels -- on a tile range behind tile 0 and on the loop path's header compare
    ("behind the stream")."""
    fr = _frame("k20", "padded")
    sA, flA = whole._recoverable("k20", "padded")
    base = [np.asarray(sA).reshape(-1), stream_of(orc, fr, "clean"), stream_of(orc, fr, "clean"), np.asarray(sA).reshape(-1)]
    wins = windows_of(len(fr.padded), 20)
    for f_bad, at, value in ((1, 5, None), (2, 40, 0xFF)):
        fs = [s.copy() for s in base]
        fs[f_bad][at] = (fs[f_bad][at] + 1) % 27 if value is None else value
        batch = Batch(gpu, fr, fs)
        for lab in ("inside one tile", "full frame", "behind the stream"):
            win = wins[lab]
            got, ver, p = batch.window(win, PIXELS)
            want = want_bytes(orc, crop_np(fr.padded, *win), PIXELS)
            for f in range(4):
                assert ver[f] == [1 if f == f_bad else 0] + words_among(fr, base[f], [], p.frame)[1:], (f_bad, lab, f, ver[f])
                bounds.check_equal(got[f], want, FILL, "header word run %d, %s, frame %d" % (f_bad, lab, f))
        batch.done()


# ---- 7. n_frames 0 and 1, w * h == 0 ----------------------------------------------------------------------------------------------------
def test_zero_and_one_frame_and_empty_window(gpu, orc):
    """n_frames = 0 launches and writes nothing -- the verdict keeps its fill, the output its own; n_frames = 1 is the single-frame
    entry, whatever the stride arguments say (0 here), at an output base that is 4-byte but not 16-byte aligned too; w * h == 0 is T3_OK
    with the verdict untouched."""
    import torch
    fr = _frame("k20", "small")
    sA, flA = whole._recoverable("k20", "small")
    frames = [np.asarray(sA).reshape(-1), stream_of(orc, fr, "clean")]
    win = (7, 44, 1, 2, 5, 42)
    for fmt in (PIXELS, RGB):
        batch = Batch(gpu, fr, frames)
        got, ver, _ = batch.window(win, fmt, n_frames=0)
        assert all((g == FILL).all() for g in got) and ver == [[SPARE] * 4] * 2, (fmt, ver)
        for empty in ((7, 44, 1, 2, 0, 42), (7, 44, 1, 2, 5, 0)):
            _, ver, p = batch.window(empty, fmt)
            assert ver == [[SPARE] * 4] * 2 and p.out_bytes == 0 and p.one_launch == 0, (fmt, empty, ver)
        batch.done()
        one = Batch(gpu, fr, frames[:1], in_stride=0)
        alone, w4 = Call(gpu, fr, frames[0]).window(win, fmt)
        got, ver, _ = one.window(win, fmt, out_stride=0)
        assert ver == [w4] == [[0, 0, flA, flA]] and np.array_equal(got[0], alone), (fmt, ver, w4)
        bounds.check_equal(got[0], want_bytes(orc, crop_np(fr.padded, *win), fmt), FILL, "one frame, fmt %d" % fmt)
        out = bounds.Buf(win[4] * win[5] * SIZE[fmt], FILL, 4, name="window at 4 mod 16")
        v = torch.full((6,), SPARE, dtype=torch.int32, device="cuda")
        gpu.decode_erasures_frames_window_async(one.inb.ptr, one.nb // 9, 1, 1, one.cfg, fr.n_raw, *win, out.ptr, 1, fmt, v.data_ptr(), torch.cuda.current_stream().cuda_stream)
        bounds.sync()
        assert v.cpu().tolist() == w4 + [SPARE] * 2 and np.array_equal(out.result(), alone), fmt
        one.done()


# ---- 8. the loop path ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("luma", "2d_64x64_k20"))
def test_loop_path(gpu, orc, name):
    """Per-band k and 2-D, three frames (recoverable, mixed with refused blocks, clean): the private copy, the erasure repair and the
    window decode of the copy frame by frame.  The words are the repair's over the WHOLE frame -- those of the whole-frame erasure
    entry --, the windows of the frames without refused blocks the crop of the frame's own pixels."""
    fr = _frame(name, "small")
    s, fl = whole._recoverable(name, "small")
    mixed = np.ascontiguousarray(ep.damage_frame(orc, fr, 45)[0], np.uint8).reshape(-1)
    frames = [np.asarray(s).reshape(-1), mixed, stream_of(orc, fr, "clean")]
    w4 = [whole.run(gpu, fr, f, PIXELS)[1] for f in frames]
    assert w4[0] == [0, 0, fl, fl] and w4[1][1] > 0 and w4[2] == [0, 0, 0, 0]
    wins = windows_of(len(fr.padded), max(fr.ks))
    batch = Batch(gpu, fr, frames, offset=2)
    for lab in ("full frame", "3 x 5", "fw = 7", "past the stream"):
        win = wins[lab]
        for fmt in (PIXELS, RGB):
            got, ver, p = batch.window(win, fmt, out_stride=round16(win[4] * win[5] * SIZE[fmt]) + 16)
            assert p.one_launch == 0 and p.frame.path == 0 and p.scratch_bytes == p.frame.scratch_bytes > 0 and p.tiles_launched == 0, (name, lab)
            assert ver == w4, (name, lab, fmt, ver, w4)
            want = want_bytes(orc, crop_np(fr.padded, *win), fmt)
            for f in (0, 2):
                bounds.check_equal(got[f], want, FILL, "loop path %s" % ((name, lab, fmt, f),))
    batch.done()


# ---- 9. the synchronous entries ---------------------------------------------------------------------------------------------------------
def sync_window(orc, fr):
    """an odd-width window of the k20 'padded' frame that starts in tiles the mixed stream of sync_batch leaves good and ends inside a
    tile it refuses: T3_E_RS shows, and most of the window is compared"""
    y0, y_good, y_in = rows_of_a_good_run(fr, far_of(orc, fr, ("damaged", 36)))
    y0 = max(y0, y_good - 20)
    return (251, -(-len(fr.padded) // 251), 20, y0, 201, y_in - y0)


def test_synchronous_entries(gpu, orc):
    """The five frames of test_gpu_decode_erasures_frames.sync_batch through the _dev and the host form at two strides: the frame whose
    header does not decode reports E_HEADER and zero counts, its output span is untouched on the device and in the host array, and it
    splits the batch into two runs; counts[4 f] is 0 although frame 1's header holds two errors; *seen is the frames' configuration; the
    inputs are unchanged.  No decodable header: E_HEADER, nothing written.  An empty window: the headers' codes, nothing launched."""
    import ctypes as C
    import torch
    fr = eframes.keep_frame(_frame("k20", "padded"))
    frames, cases, want_rc, _ = eframes.sync_batch(gpu, orc, fr)
    nb, N = len(frames[0]), len(frames)
    win = sync_window(orc, fr)
    ob = win[4] * win[5] * 6
    one = gpu.decode_erasures_window_plan(fr.n_raw, gpu.make_cfg(mode=1, **fr.kw), *win, PIXELS)
    assert one.path == 1 and 0 < one.tiles_launched < one.win.n_tiles and one.win.tile_lo > 0
    fars = [far_of(orc, fr, c) if c is not None else [] for c in cases]
    keeps = mask_conditions(fr, fars, win, "sync")
    want_counts = [words_among(fr, stream_of(orc, fr, c), far, one) if c is not None else [0] * 4 for c, far in zip(cases, fars)]
    want_rc = [gpu.E_HEADER if c is None else gpu.E_RS if w[1] else gpu.OK for c, w in zip(cases, want_counts)]
    assert any(w[2] > 0 for w in want_counts)
    wants = [want_bytes(orc, crop_np(eframes._pixels(fr.name, fr.n_px, c), *win), PIXELS) if c is not None else None for c in cases]
    st = torch.cuda.current_stream().cuda_stream
    for in_stride, out_stride in ((nb + (nb & 1), round16(ob)), (round16(nb) + 32, round16(ob) + 32)):
        data, _ = layout(frames, in_stride)
        spans = tuple((f * out_stride, f * out_stride + ob) for f in range(N))
        inb = bounds.Buf(len(data), FILL, 2, data=data, name="coded batch")
        out = bounds.Buf(0, FILL, 0, data=np.full(spans[-1][1], FILL, np.uint8), name="window batch", may_change=[spans[f] for f in range(N) if cases[f] is not None])
        seen = gpu.DecoderContext(mode=1).cfg_last_seen
        rc, rcs, counts = gpu.decode_erasures_frames_window_dev(inb.ptr, nb // 9, in_stride, N, seen, *win, out.ptr, out_stride, PIXELS, st)
        bounds.sync()
        assert rc == gpu.OK and rcs == want_rc and counts == want_counts, (in_stride, rc, rcs, counts, want_counts)
        assert seen.profile == rp.CONFIGS["k20"]["profile"] and seen.mode == 1
        inb.result()
        got = out.result()                                                  # the E_HEADER frame's span is no may_change range: untouched
        for f, c in enumerate(cases):
            if c is not None:
                check_masked(got[spans[f][0]: spans[f][1]], wants[f], keeps[f], PIXELS, FILL, ("dev", in_stride, f))
        w, _ = layout(frames, in_stride)
        w = np.concatenate([w, np.full(in_stride - nb, 0x3C, np.uint8)]).reshape(N, in_stride)
        before = w.copy()
        ctx = gpu.DecoderContext(mode=1)
        rc, rcs, outs, counts = gpu.decode_erasures_frames_window(w, ctx, *win, PIXELS)
        assert rc == gpu.OK and rcs == want_rc and counts == want_counts and np.array_equal(w, before), (in_stride, "host", rc, rcs, counts)
        assert ctx.cfg_last_seen.profile == rp.CONFIGS["k20"]["profile"]
        for f, c in enumerate(cases):
            if c is None:
                assert outs[f] is None
            else:
                check_masked(np.ascontiguousarray(outs[f]).view(np.uint8).reshape(-1), wants[f], keeps[f], PIXELS, FILL, ("host", in_stride, f))
    # the host entry itself: a refused frame's span of the caller's output array stays as it was, and so does a stride gap
    flat, _ = layout(frames, nb + (nb & 1))
    hos = ob + 10
    hout = np.full(N * hos, 0xEE, np.uint8); cnt = (C.c_uint32 * (4 * N))(); rcs = (C.c_int * N)()
    ctx = gpu.DecoderContext(mode=1)
    rc = gpu.lib().t3hip_decode_erasures_frames_window(flat.ctypes.data_as(C.c_void_p), C.c_uint64(nb // 9), C.c_uint64(nb + (nb & 1)), C.c_uint32(N), C.byref(ctx.cfg_last_seen),
                                                       *[C.c_uint32(x) for x in win], hout.ctypes.data_as(C.c_void_p), C.c_uint64(hos), C.c_int(PIXELS), cnt, rcs)
    hout = hout.reshape(N, hos)
    assert rc == gpu.OK and list(rcs) == want_rc and (hout[2] == 0xEE).all() and (hout[:, ob:] == 0xEE).all()
    bounds.check_equal(hout[4, :ob], wants[4], 0xEE, "host entry, last frame")
    # no header decodes: E_HEADER, nothing written
    bad = [whole._damage_header(frames[0], 9)] * 2
    data, _ = layout(bad, nb + (nb & 1))
    inb = bounds.Buf(len(data), FILL, 0, data=data, name="coded batch"); out = bounds.Buf(round16(ob) + ob, FILL, 0, name="window batch")
    rc, rcs, counts = gpu.decode_erasures_frames_window_dev(inb.ptr, nb // 9, nb + (nb & 1), 2, gpu.DecoderContext(mode=1).cfg_last_seen, *win, out.ptr, round16(ob), PIXELS, st)
    bounds.sync()
    assert rc == gpu.E_HEADER and rcs == [gpu.E_HEADER] * 2 and counts == [[0] * 4] * 2
    inb.result(); out.untouched()
    rc, rcs, outs, counts = gpu.decode_erasures_frames_window(np.stack(bad), gpu.DecoderContext(mode=1), *win, PIXELS)
    assert rc == gpu.E_HEADER and rcs == [gpu.E_HEADER] * 2 and counts == [[0] * 4] * 2 and outs == [None, None]
    # seen->mode must be FIXED on entry
    with pytest.raises(gpu.T3Error) as e:
        gpu.decode_erasures_frames_window(np.stack(frames), gpu.DecoderContext(mode=0), *win, PIXELS)
    assert e.value.code == gpu.E_ARG
    # an empty window: the headers are parsed, nothing is launched or written
    data, _ = layout(frames, nb + (nb & 1))
    inb = bounds.Buf(len(data), FILL, 0, data=data, name="coded batch"); out = bounds.Buf(64, FILL, 0, name="window batch")
    seen = gpu.DecoderContext(mode=1).cfg_last_seen
    rc, rcs, counts = gpu.decode_erasures_frames_window_dev(inb.ptr, nb // 9, nb + (nb & 1), N, seen, 251, win[1], 20, win[3], 0, 30, out.ptr, 16, PIXELS, st)
    bounds.sync()
    assert rc == gpu.OK and rcs == [gpu.E_HEADER if c is None else gpu.OK for c in cases] and counts == [[0] * 4] * N and seen.profile == rp.CONFIGS["k20"]["profile"]
    inb.result(); out.untouched()


def two_configuration_batch(t3, orc):
    """A A B B A of test_gpu_repair_frames.two_configurations on the odd-sized k20 frame -> (the frames' Frame objects, their received
    streams, the yardstick's (R', six words, refused blocks) of each, the window)"""
    from test_gpu_repair_frames import two_configurations
    A, B = two_configurations(t3, orc, eframes._small_odd(t3, orc, "k20").n_px)
    order = (A, A, B, B, A)
    adm = list(ep.admissible(A.ks[0]))
    received = [ep.damage_frame(orc, A, 91, only=adm)[0], A.clean.reshape(-1), ep.damage_frame(orc, B, 92, only=eframes._kinds(B, 92))[0], ep.damage_frame(orc, B, 93, only=adm)[0], None]
    received[4] = received[0]
    frames = [np.ascontiguousarray(s, np.uint8).reshape(-1) for s in received]
    yard = [ep.expected_erasures(orc, fr, s) for fr, s in zip(order, frames)]
    fw = 251; fh = -(-len(A.padded) // fw)
    y0, _, y_in = rows_of_a_good_run(B, yard[2][2])                          # from the tiles frame 2 leaves good into one it refuses
    return order, frames, yard, (fw, fh, 0, y0, fw, y_in - y0)


def test_two_configurations_in_one_batch(gpu, orc):
    """A A B B A: five frames of one profile and one n_raw_words whose scrambler seeds differ, through the _dev and the host entry.  The
    runs are 2, 2, 1 -- the one launch twice and the single-frame body inside a batch -- and every frame's window (outside the tiles of
    its refused blocks), counts and code are the yardstick's for that frame alone."""
    import torch
    order, frames, yard, win = two_configuration_batch(gpu, orc)
    A = order[0]
    cfg = gpu.make_cfg(mode=1, **A.kw)
    one = gpu.decode_erasures_window_plan(A.n_raw, cfg, *win, PIXELS)
    assert gpu.decode_erasures_frames_window_plan(A.n_raw, 2, cfg, *win, PIXELS).one_launch == 1 and one.tiles_launched >= 2
    fars = [far for _, _, far in yard]
    keeps = mask_conditions(A, fars, win, "two configurations")
    want_counts = [words_among(fr, s, far, one) for fr, s, far in zip(order, frames, fars)]
    want_rc = [gpu.E_RS if c[1] else gpu.OK for c in want_counts]
    assert gpu.OK in want_rc and want_counts[0][2] > 0 and want_counts[2] != want_counts[0] and want_counts[1] == [0] * 4, (want_rc, want_counts)
    wants = [want_bytes(orc, crop_np(whole.expected_pixels(orc, fr, e, far), *win), PIXELS) for fr, (e, _, far) in zip(order, yard)]
    nb, N = len(frames[0]), len(frames)
    ob = win[4] * win[5] * 6
    in_stride, out_stride = nb + (nb & 1), round16(ob)
    data, _ = layout(frames, in_stride)
    spans = tuple((f * out_stride, f * out_stride + ob) for f in range(N))
    inb = bounds.Buf(len(data), FILL, 2, data=data, name="coded batch")
    out = bounds.Buf(0, FILL, 0, data=np.full(spans[-1][1], FILL, np.uint8), name="window batch", may_change=spans)
    seen = gpu.DecoderContext(mode=1).cfg_last_seen
    rc, rcs, counts = gpu.decode_erasures_frames_window_dev(inb.ptr, nb // 9, in_stride, N, seen, *win, out.ptr, out_stride, PIXELS, torch.cuda.current_stream().cuda_stream)
    bounds.sync()
    assert rc == gpu.OK and rcs == want_rc and counts == want_counts, (rc, rcs, counts, want_counts)
    inb.result()
    got = out.result()
    for f, (lo, hi) in enumerate(spans):
        check_masked(got[lo:hi], wants[f], keeps[f], PIXELS, FILL, ("two configurations, dev", f))
    w, _ = layout(frames, in_stride)
    w = np.concatenate([w, np.full(in_stride - nb, 0x3C, np.uint8)]).reshape(N, in_stride)
    before = w.copy()
    rc, rcs, outs, counts = gpu.decode_erasures_frames_window(w, gpu.DecoderContext(mode=1), *win, PIXELS)
    assert rc == gpu.OK and rcs == want_rc and counts == want_counts and np.array_equal(w, before), ("host", rc, rcs, counts)
    for f in range(N):
        check_masked(np.ascontiguousarray(outs[f]).view(np.uint8).reshape(-1), wants[f], keeps[f], PIXELS, FILL, ("two configurations, host", f))


def test_decode_frames_window_erasures_demo(gpu, orc, tmp_path):
    """tests/cpp/decode_frames_window_erasures_demo.cpp: a viewer's crop out of every frame of a received run through
    decode_frames_window_erasures of include/ternary_codec_v6.hpp, built with g++ alone: three frames (recoverable, header damaged
    beyond t, clean) give the crop of the frame's own pixels for the first and the last and no pixels for the second."""
    lib = os.path.join(ROOT, "ternary-image-codec_amd")
    exe = str(tmp_path / "decode_frames_window_erasures_demo")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "decode_frames_window_erasures_demo.cpp"),
                    "-L" + lib, "-lt3hip", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-o", exe], check=True)
    fr = _frame("k20", "small")
    s, flagged = whole._recoverable("k20", "small")
    s = np.asarray(s).reshape(-1)
    win = (7, 44, 1, 2, 5, 42)
    fin, fout = str(tmp_path / "in.words"), str(tmp_path / "out.px")
    np.concatenate([s, whole._damage_header(s, 9), stream_of(orc, fr, "clean")]).tofile(fin)
    out = json.loads(subprocess.run([exe, fin, "3"] + [str(x) for x in win] + [fout], check=True, capture_output=True, text=True).stdout)
    assert out == {"ok": 1, "frames": [{"status": 0, "counts": [0, flagged, flagged]}, {"status": gpu.E_HEADER, "counts": [0, 0, 0]}, {"status": 0, "counts": [0, 0, 0]}]}, out
    want = crop_np(fr.padded, *win).view(np.uint8)
    got = np.fromfile(fout, np.uint8).reshape(3, -1)
    assert np.array_equal(got[0], want) and np.array_equal(got[2], want) and not got[1].any()


# every (frame, refused blocks per frame, window) a test above compares outside refused tiles: f(t3, orc) -> [(tag, frame, fars, win)],
# for tests/test_decode_erasures_frames_window_plan.py, which proves mask_conditions on them with the yardstick alone
def _masked_mixed(t3, orc):
    out = []
    for name in FUSED:
        fr, _, fars, wins = mixed_batch(orc, name)
        out += [(("mixed", name, lab), fr, fars, win) for lab, win in wins.items()]
    return out


def _masked_addresses(t3, orc):
    out = []
    for name in ("k20", "k20_beacon83"):
        fr, _, fars, wins = address_batch(t3, orc, name)
        out += [(("addresses", name, lab), fr, fars, win) for lab, win in wins.items()]
    return out


def _masked_crossing(t3, orc):
    out = []
    for name in ("k20", "k20_beacon83"):
        fr, _, fars = crossing_batch(t3, orc, name)
        out += [(("crossing", name, win), fr, fars, win) for win in crossing_windows(name)]
    return out


def _masked_sync(t3, orc):
    fr = eframes.keep_frame(_frame("k20", "padded"))
    _, cases, _, _ = eframes.sync_batch(t3, orc, fr)
    out = [(("sync",), fr, [far_of(orc, fr, c) if c is not None else [] for c in cases], sync_window(orc, fr))]
    order, _, yard, win = two_configuration_batch(t3, orc)
    return out + [(("two configurations",), order[0], [far for _, _, far in yard], win)]


MASKED = (_masked_mixed, _masked_addresses, _masked_crossing, _masked_sync)
