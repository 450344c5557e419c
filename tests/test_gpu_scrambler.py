"""Every scrambler sequence through every encoder and decoder path.

The kernels never run the scrambler's recurrence: they read ScrCycle (t3_host.hpp) -- two pre-period states and a 6-periodic tail -- in
many derived forms (pattern rows with a special row for the stream's first block, the matrix-core table per parity phase, the LUT variant
bases, `first` patches, scr_state / rp_scr_state, the 48-bit replicated form of the descramble stage).  The default seed (1, 1, 1) gives
2, 0, 1, 2, 0, 1, ...: a phase that is wrong by three, a `first` flag that never fires or fires for the wrong block, a special row built
from the tail alone all go unseen under it.  tests/scrambler_seqs.py enumerates the whole space: 27 next-maps x 3 start states = 81 seeds in
21 sequence classes (3 constant, 6 of period 2, 6 of period 3, 6 transient x, y, y, y, ...).  Every cell below runs all 21 classes, the
large frames all 81 seeds, and compares bytes with the CPU oracle (or with the pixels the oracle encoded).

Frames (scrambler_seqs.frame_sizes): one word; two words with an odd pixel count; right behind the first tile boundary, odd; about
frame_ends.CAP symbols -- at least three tiles of every kernel with a ragged last one.  Decoded streams carry 0 .. t errors in every block
at the band's own t and t errors in block 0 of band 0 that include body symbols 0 and 1; a second stream has its t errors right behind
those two symbols, so that one wrong state there is more than the code corrects; a third has an uncorrectable block there.
tests/test_scrambler_sequences.py proves on the CPU what the oracle says of each of them."""
import json
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import frame_ends as fe
import oracle_lib as ol
import rs_patterns as rp
import scrambler_seqs as ss
from test_decode_stages import KS, restate_stage3, stage_body
from test_gpu_fixed_errors import KNOBS, OUTPUTS
from test_gpu_frames import decode_batch, encode_batch
from test_gpu_frames_window import Batch, batch_window, encode_images, images_of
from test_gpu_repair import run as run_repair
from test_gpu_window import crop_np
from test_oracle_vs_ref import decoder_consistent_stream
from test_repair_semantics import FUSED, SWEEP

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRONT_ENDS = ("pixels", "rgb", "words")
OTHER = ("k20", "k18", "luma", "k20_beacon83", "2d_64x64_k20", "four_codes")
ALL_CLASSES = list(range(21))


def st():
    import torch
    return torch.cuda.current_stream().cuda_stream


def up(a):
    import torch
    return torch.from_numpy(np.array(fe.u8(a), copy=True)).cuda()


def entry(gpu, front_end):
    return {"pixels": gpu.encode_frame_dev, "rgb": gpu.encode_rgb_dev, "words": gpu.encode_profile_dev}[front_end]


def seen_dict(c):
    d = c.as_dict(); d.pop("mode"); return d


class Seeds:
    """Runs a cell's body seed by seed and fails at the end, naming every seed whose body failed and the kinds of their sequences: a
    failure report then says which sequence classes a fault shows under.  (Only assertions are collected; an error of a call ends the test.)"""

    def __init__(self):
        self.bad = []

    def run(self, seed, body):
        try:
            body()
        except AssertionError as e:
            self.bad.append((tuple(seed), ss.SEQUENCES[ss.class_of(seed)].kind, (str(e).splitlines() or [""])[0][:200]))

    def done(self):
        kinds = sorted({b[1] for b in self.bad})
        assert not self.bad, "%d of the runs failed; kinds of sequence: %s; classes: %s; first: %s" % (len(self.bad), kinds, ss.classes([b[0] for b in self.bad]), self.bad[0])


# ---- encoders ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,mode", [(n, m) for n in ss.ENC_FRAMINGS for m in (0, 1)])
def test_encoders(gpu, orc, name, mode):
    """t3hip_encode_frame (host), _frame_dev, _profile_dev (raw words) and _rgb_dev, COMPAT and FIXED: all 81 seeds at the largest size, the
    21 representatives at the three small ones.  Every byte of the stream is the oracle's, nothing is written behind it."""
    import torch
    runs = Seeds()
    for size in ss.SIZES:
        ec = ss.enc_case(name, mode, size)
        seeds = ss.seeds_at(size)
        assert ss.classes(seeds) == ALL_CLASSES
        want = {f: ec.want(f, seeds) for f in ("pixels", "words")}
        want["rgb"] = want["pixels"]
        src = {f: up(ec.data(f)[0]) for f in FRONT_ENDS}
        cap = len(want["pixels"][0]) // 9
        outs = {f: torch.empty(9 * cap + 64, dtype=torch.uint8, device="cuda") for f in FRONT_ENDS}
        def one(i, seed):
            cfg = gpu.make_cfg(mode=mode, **dict(ec.kw, seed=seed))
            assert gpu.encoded_words(ec.W, cfg) == cap
            for f in FRONT_ENDS:
                outs[f].fill_(0xA5)
                n = entry(gpu, f)(src[f].data_ptr(), ec.data(f)[1], cfg, outs[f].data_ptr(), cap, st())
                assert n == cap, (name, mode, size, seed, f, n)
            torch.cuda.synchronize()
            for f in FRONT_ENDS:
                got = outs[f].cpu().numpy()
                assert np.array_equal(got[: 9 * cap], want[f][i]), (name, mode, size, seed, f, ss.SEQUENCES[ss.class_of(seed)].kind)
                assert (got[9 * cap:] == 0xA5).all(), (name, mode, size, seed, f)
            ok, host = gpu.encode_frame(ec.px, cfg)
            assert ok and np.array_equal(fe.u8(host), want["pixels"][i]), (name, mode, size, seed, "host")
        for i, seed in enumerate(seeds):
            runs.run(seed, lambda: one(i, seed))
    runs.done()


@pytest.mark.parametrize("name,mode", [(n, m) for n in ss.ENC_FRAMINGS for m in (0, 1)])
def test_batched_encoders(gpu, orc, name, mode):
    """t3hip_encode_frames_dev, three different frames, pixel, raw-word and RGB input, the 21 representatives (the second ones at the
    small size): frames 1 and 2 show the pre-period states exactly as frame 0 does -- each is the oracle's stream of its own content.  The
    largest size has at least three encoder tiles per frame (an encoder tile is at most 12096 symbols): a per-frame phase that is wrong
    from tile 1 on shows there."""
    runs = Seeds()
    for size, seeds in (("w2", ss.REPS2), ("tile", ss.REPS), ("cap", ss.REPS)):
        assert ss.classes(seeds) == ALL_CLASSES
        ecs = [ss.enc_case(name, mode, size, salt) for salt in (0, 1, 2)]
        for fmt, f in ((gpu.FRAMES_PIXELS, "pixels"), (gpu.FRAMES_WORDS, "words"), (gpu.FRAMES_RGB, "rgb")):
            want = [ec.want(f, seeds) for ec in ecs]
            def one(i, seed):
                cfg = gpu.make_cfg(mode=mode, **dict(ecs[0].kw, seed=seed))
                p, got = encode_batch(gpu, [ec.data(f)[0] for ec in ecs], ecs[0].data(f)[1], fmt, cfg, 0)
                w = ss.batch_encode_one_launch(name, mode, size, f)                # the batch kernel: `first` per frame, not per launch
                assert w is None or p.one_launch == w, (name, mode, size, f)
                for q in range(3):
                    assert np.array_equal(got[q], want[q][i]), (name, mode, size, seed, f, "frame %d" % q, ss.SEQUENCES[ss.class_of(seed)].kind)
            for i, seed in enumerate(seeds):
                runs.run(seed, lambda: one(i, seed))
    runs.done()


# ---- FIXED decoders ------------------------------------------------------------------------------------------------------------------
class Dec:
    """Output and verdict buffers for frames of up to n_raw words, and the two device entries."""

    def __init__(self, gpu, n_raw):
        import torch
        self.gpu, self.t = gpu, torch
        self.out = torch.empty(12 * n_raw + 64, dtype=torch.uint8, device="cuda")
        self.ver = torch.empty(2, dtype=torch.int32, device="cuda")

    def run_async(self, d, cfg, n_raw, to_pixels):
        n, sz = (2 * n_raw, 6) if to_pixels else (n_raw, 9)
        self.out.fill_(0xA5); self.ver.fill_(7)
        got = self.gpu.decode_frame_async(d.data_ptr(), d.numel() // 9, cfg, n_raw, self.out.data_ptr(), n, self.ver.data_ptr(), to_pixels, st())
        self.t.cuda.synchronize()
        assert got == n
        return self.ver.cpu().tolist(), self.out[: n * sz].cpu().numpy()

    def run_sync(self, d, n_raw, to_pixels):
        n, sz = (2 * n_raw, 6) if to_pixels else (n_raw, 9)
        self.out.fill_(0xA5)
        seen = self.gpu.DecoderContext(mode=1).cfg_last_seen
        rc, got = self.gpu.decode_profile_dev(d.data_ptr(), d.numel() // 9, seen, self.out.data_ptr(), n, to_pixels, st())
        self.t.cuda.synchronize()
        return rc, got == n, seen, self.out[: n * sz].cpu().numpy()


def oracle_seen(orc, fr):
    """What the oracle remembers of the frame's header: the seeds mod 27 among it."""
    seen = ol.make_cfg(mode=1)
    assert orc.decode_frame(fr.clean, seen)[0] == 0
    assert (seen.seed_a, seen.seed_b, seen.seed_s0) == tuple(x % 27 for x in fr.scr)
    return seen_dict(seen)


def check_frame(gpu, orc, dec, fr, outputs, label, sync=True):
    """One DecFrame through t3hip_decode_frame_async (the caller's full seeds) and t3hip_decode_profile_dev (what the header carries):
    pixels / raw words and verdict [0, 0] for the two <= t streams, verdict [0, 1] / T3_E_RS for the stream with the far block."""
    tag = (label, fr.size, fr.scr, ss.SEQUENCES[ss.class_of(fr.scr)].kind)
    cfg = gpu.make_cfg(mode=1, **fr.kw)
    want = dict(zip((True, False), fr.want()))
    good, d_far = (("le_t", up(fr.le_t())), ("tight", up(fr.tight()))), up(fr.far())
    oseen = oracle_seen(orc, fr) if sync else None
    for to_pixels in outputs:
        for what, d_ok in good:
            ver, got = dec.run_async(d_ok, cfg, fr.n_raw, to_pixels)
            assert ver == [0, 0], (tag, what, to_pixels, ver)
            assert np.array_equal(got, want[to_pixels]), (tag, what, to_pixels, "async")
        ver, _ = dec.run_async(d_far, cfg, fr.n_raw, to_pixels)
        assert ver == [0, 1], (tag, to_pixels, "far", ver)
        if sync:
            for what, d_ok in good:
                rc, full, seen, got = dec.run_sync(d_ok, fr.n_raw, to_pixels)
                assert rc == 0 and full and np.array_equal(got, want[to_pixels]), (tag, what, to_pixels, "sync", rc)
                assert seen_dict(seen) == oseen, (tag, seen_dict(seen), oseen)
            assert dec.run_sync(d_far, fr.n_raw, to_pixels)[0] == gpu.E_RS, (tag, to_pixels, "sync far")


@pytest.mark.parametrize("name", list(rp.CONFIGS))
def test_fixed_decoders(gpu, orc, name):
    """Every framing of rs_patterns.CONFIGS (fused kernel with and without a beacon, one-launch UEP / 2-D kernel, two-kernel decoder for raw
    words, four codes and 7 x 5 tiles), the outputs of test_gpu_fixed_errors.OUTPUTS: all 81 seeds at the largest size, 21 elsewhere."""
    runs = Seeds()
    for size in ss.SIZES:
        seeds = ss.seeds_at(size)
        assert ss.classes(seeds) == ALL_CLASSES
        frames = ss.dec_frames(gpu, name, size, seeds)
        dec = Dec(gpu, frames[0].n_raw)
        for fr in frames:
            cfg = gpu.make_cfg(mode=1, **fr.kw)                                        # the fused kernel's framings, as the planners name them
            assert gpu.window_plan(fr.n_raw, cfg, 2 * fr.n_raw, 1, 0, 0, 2 * fr.n_raw, 1).tile_range == ss.TILE_RANGE[name]
            assert gpu.frames_plan(True, 2 * fr.n_raw, 2, cfg, gpu.FRAMES_PIXELS).one_launch == ss.TILE_RANGE[name]
            runs.run(fr.scr, lambda: check_frame(gpu, orc, dec, fr, OUTPUTS[name], name))
    runs.done()


@pytest.mark.parametrize("knob,name", KNOBS)
def test_fixed_decoders_forced_paths(gpu, orc, knob, name):
    """The generic gather decoder (scr_state) and the two-kernel decoder (`first` of t3_decode_fx.h) forced by their knobs."""
    frames = [fr for size in ss.SIZES for fr in ss.dec_frames(gpu, name, size, ss.REPS2 if size == "w2" else ss.REPS)]
    assert ss.classes([fr.scr for fr in frames if fr.size == "cap"]) == ALL_CLASSES
    dec = Dec(gpu, max(fr.n_raw for fr in frames))
    runs = Seeds()
    os.environ[knob] = "1"
    try:
        for fr in frames:
            runs.run(fr.scr, lambda: check_frame(gpu, orc, dec, fr, OUTPUTS[name], "%s %s" % (knob, name)))
    finally:
        os.environ.pop(knob, None)
    runs.done()


HDR_NAMES = ("k20", "luma", "four_codes")


def _hdr_kernel_cases(t3):
    """Both <= t streams and the far stream of the 21 representatives (size `tile`) through t3hip_decode_frame_async ->
    {framing: [[verdict, crc32 of the pixels (le_t), verdict, crc32 of the pixels (tight), verdict of the far stream] per class]}"""
    out = {}
    for name in HDR_NAMES:
        frames = ss.dec_frames(t3, name, "tile", ss.REPS)
        dec = Dec(t3, frames[0].n_raw); rows = []
        for fr in frames:
            cfg = t3.make_cfg(mode=1, **fr.kw); row = []
            for s in (fr.le_t(), fr.tight()):
                ver, got = dec.run_async(up(s), cfg, fr.n_raw, True)
                row += [ver, zlib.crc32(got.tobytes())]
            rows.append(row + [dec.run_async(up(fr.far()), cfg, fr.n_raw, True)[0]])
        out[name] = rows
    return out


_HDR_CHILD = r"""
import json, os, sys
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import __graft_entry__ as ge
from test_gpu_scrambler import _hdr_kernel_cases
t3 = ge.load_package(); t3.init(0)
print("cases " + json.dumps(_hdr_kernel_cases(t3)))
"""


def test_fixed_decoders_header_kernel(gpu, orc):
    """T3HIP_HDR_KERNEL=1 (read once per process: a child of its own): the header check as a launch in front of the decoder instead of
    folded into it, on the fused, the one-launch UEP and the two-kernel path.  Expected: the oracle's pixels, not this process's.  The
    `tight` stream is what sees a wrong pre-period state where t >= 2 (k20, luma)."""
    want = {name: [2 * [[0, 0], zlib.crc32(fr.want()[0].tobytes())] + [[0, 1]] for fr in ss.dec_frames(gpu, name, "tile", ss.REPS)] for name in HDR_NAMES}
    env = dict(os.environ, T3HIP_HDR_KERNEL="1")
    r = subprocess.run([sys.executable, "-c", "ROOT = %r\n" % ROOT + _HDR_CHILD], env=env, capture_output=True, text=True, timeout=600)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("cases ")]
    assert r.returncode == 0 and lines, r.stdout[-2000:] + r.stderr[-4000:]
    got = json.loads(lines[0][len("cases "):])
    for name in HDR_NAMES:
        for i, (g, w) in enumerate(zip(got[name], want[name])):
            assert g == w, (name, ss.SEQUENCES[i], g, w)


# ---- the other entries ---------------------------------------------------------------------------------------------------------------
def check_window_plan(p, name, size, label, tag):
    """The launch the window gets is the one the expectation is written for (scrambler_seqs.TILE_RANGE, far_verdict: set down there, not
    taken from the plan; tests/test_scrambler_sequences.py::test_plans holds the planner against them on the CPU too)."""
    assert p.tile_range == ss.TILE_RANGE[name], (tag, label, p.tile_range)
    if p.tile_range:
        assert (p.tile_lo >= 1) == ss.starts_behind_tile0(name, size, label) and p.tile_hi > p.tile_lo, (tag, label, p.tile_lo, p.tile_hi)


@pytest.mark.parametrize("name", OTHER)
def test_other_entries(gpu, orc, name):
    """t3hip_decode_rgb_async, the host t3hip_decode_frame and t3hip_decode_profile, t3hip_decode_window_async over the whole frame, over a
    window whose tile range starts at tile >= 1 and over one at tile 0: the launch's first tile gets the first block's treatment only if
    it is the stream's.  21 representatives at the largest size, the second ones at two words; both <= t streams and the far one."""
    import torch
    runs = Seeds()

    def one(fr, size):
        tag = (name, size, fr.scr, ss.SEQUENCES[ss.class_of(fr.scr)].kind)
        cfg = gpu.make_cfg(mode=1, **fr.kw)
        far_s = fr.far(); d_far = up(far_s)
        n = 2 * fr.n_raw; n_in = d_far.numel() // 9
        px_b, raw_b = fr.want()
        oseen = oracle_seen(orc, fr)
        ver = torch.empty(2, dtype=torch.int32, device="cuda")
        ok, back = gpu.decode_frame(far_s, gpu.DecoderContext(mode=1))
        assert not ok and len(back) == 0, (tag, "host far")
        for what, ok_s in (("le_t", fr.le_t()), ("tight", fr.tight())):
            d_ok = up(ok_s)
            # RGB out, the frame's own pixel count
            rgb = torch.full((3 * fr.n_px + 64,), 0xA5, dtype=torch.uint8, device="cuda")
            for d, v in ((d_far, [0, 1]), (d_ok, [0, 0])):
                ver.fill_(7)
                gpu.decode_rgb_async(d.data_ptr(), n_in, cfg, fr.n_px, rgb.data_ptr(), ver.data_ptr(), st())
                torch.cuda.synchronize()
                assert ver.cpu().tolist() == v, (tag, what, "rgb", v)
            got = rgb.cpu().numpy()
            assert np.array_equal(got[: 3 * fr.n_px], orc.quant_to_rgb(fr.padded[: fr.n_px])) and (got[3 * fr.n_px:] == 0xA5).all(), (tag, what, "rgb")
            # the host entries: what the header carries
            dctx = gpu.DecoderContext(mode=1)
            ok, back = gpu.decode_frame(ok_s, dctx)
            assert ok and np.array_equal(fe.u8(back), px_b), (tag, what, "host pixels")
            assert seen_dict(dctx.cfg_last_seen) == oseen, (tag, "host seen")
            ok, words = gpu.decode_profile_to_raw(ok_s, gpu.DecoderContext(mode=1))
            assert ok and np.array_equal(fe.u8(words), raw_b), (tag, what, "host words")
            # windows
            for label, win in ss.windows_of(n):
                check_window_plan(gpu.window_plan(fr.n_raw, cfg, *win), name, size, label, tag)
                crop = crop_np(fr.padded, *win)
                for fmt, sz, want in ((gpu.WINDOW_PIXELS, 6, fe.u8(crop)), (gpu.WINDOW_RGB, 3, orc.quant_to_rgb(crop))):
                    nb = win[4] * win[5] * sz
                    out = torch.full((nb + 64,), 0xA5, dtype=torch.uint8, device="cuda")
                    for d, v in ((d_far, ss.far_verdict(name, size, label)), (d_ok, [0, 0])):
                        ver.fill_(7)
                        gpu.decode_window_async(d.data_ptr(), n_in, cfg, fr.n_raw, *win, out.data_ptr(), fmt, ver.data_ptr(), st())
                        torch.cuda.synchronize()
                        assert ver.cpu().tolist() == v, (tag, what, label, fmt, v)
                    got = out.cpu().numpy()
                    assert np.array_equal(got[:nb], want) and (got[nb:] == 0xA5).all(), (tag, what, label, fmt)

    for size, seeds in (("w2", ss.REPS2), ("cap", ss.REPS)):
        assert ss.classes(seeds) == ALL_CLASSES
        for fr in ss.dec_frames(gpu, name, size, seeds):
            runs.run(fr.scr, lambda: one(fr, size))
    runs.done()


@pytest.mark.parametrize("name", ss.BATCH_DEC)
def test_batched_decoders(gpu, orc, name):
    """t3hip_decode_frames_async and t3hip_decode_frames_window_async, three different frames (k20: one launch; luma: the loop of the
    single-frame entries): frame 0 with t errors at body symbols 0, 1, .., frame 1 with the far block -- verdict words
    [0, 0, 0, 1, 0, 0] -- and frame 2 with t errors right behind symbols 0 and 1; frames 0 and 2 give their pixels."""
    runs = Seeds()

    def one(frs, size):
        seed = frs[0].scr
        tag = (name, size, seed, ss.SEQUENCES[ss.class_of(seed)].kind)
        cfg = gpu.make_cfg(mode=1, **frs[0].kw); n_raw = frs[0].n_raw
        coded = ss.batch_streams(frs)
        for fmt in (gpu.FRAMES_PIXELS, gpu.FRAMES_RGB):
            p, seen, out, ver = decode_batch(gpu, coded, n_raw, fmt, cfg, 0)
            assert p.one_launch == ss.TILE_RANGE[name] and ver == [0, 0, 0, 1, 0, 0], (tag, fmt, ver)
            for q in (0, 2):
                want = fe.u8(frs[q].padded) if fmt == gpu.FRAMES_PIXELS else orc.quant_to_rgb(frs[q].padded)
                assert np.array_equal(out[q], want), (tag, fmt, "frame %d" % q)
        b = Batch(gpu, [(up(c), len(c) // 9, cfg, frs[0].L) for c in coded], host=False)
        for label, win in ss.windows_of(2 * n_raw)[1:]:
            p = gpu.frames_window_plan(n_raw, 3, cfg, *win, gpu.WINDOW_PIXELS)
            check_window_plan(p.win, name, size, label, tag)
            assert p.one_launch == ss.TILE_RANGE[name], (tag, label)
            wins, ver = batch_window(gpu, b, n_raw, win, gpu.WINDOW_PIXELS)
            assert ver == [0, 0] + ss.far_verdict(name, size, label) + [0, 0], (tag, label, ver)
            for q in (0, 2):
                assert np.array_equal(wins[q], fe.u8(crop_np(frs[q].padded, *win))), (tag, label, "frame %d" % q)

    assert name in ss.BATCH_DEC
    for size, seeds in ss.BATCH_SIZES:
        assert ss.classes(seeds) == ALL_CLASSES
        sets = ss.batch_sets(gpu, name, size, seeds)
        for i, seed in enumerate(seeds):
            runs.run(seed, lambda: one([x[i] for x in sets], size))
    runs.done()


def test_image_batches(gpu, orc):
    """t3hip_encode_images_dev and t3hip_decode_images_async, three sources of 100 x 75 into S15 frames (854 x 480, one launch each way),
    the 21 representatives: every coded frame is the oracle's; decoded with t errors at the head of frames 0 and 2 (frame 2: none at body
    symbols 0 and 1) and a far block at the head of frame 1, images 0 and 2 are the oracle's bridge of their pixels and the verdict words
    [0, 0, 0, 1, 0, 0]."""
    ic = ss.image_case(gpu)
    assert ss.classes(ss.REPS) == ALL_CLASSES
    ic.prefetch(ss.REPS)
    runs = Seeds()

    def one(seed):
        tag = (seed, ss.SEQUENCES[ss.class_of(seed)].kind)
        cfg = gpu.make_cfg(mode=1, **dict(ss.IMG_KW, seed=seed))
        assert gpu.frames_plan(False, 854 * 480, 3, cfg, gpu.FRAMES_RGB).one_launch == 1
        assert gpu.frames_window_plan(ic.n_raw, 3, cfg, 854, 480, 0, 0, 854, 480, gpu.WINDOW_RGB).one_launch == 1
        got, n_enc = encode_images(gpu, ic.srcs, ss.IMG_SUB, False, cfg)
        for f, want in enumerate(ic.coded(seed)):
            assert np.array_equal(got[f].cpu().numpy(), want), (tag, "encode, frame %d" % f)
        b = Batch(gpu, [(up(c), n_enc, cfg, None) for c in ic.damaged(seed)], host=False)
        imgs, ver = images_of(gpu, b, ss.IMG_SUB, False, 16)
        assert ver == [0, 0, 0, 1, 0, 0], (tag, ver)
        for f in (0, 2):
            assert np.array_equal(imgs[f].cpu().numpy(), ic.rgb[f]), (tag, "decode, image %d" % f)

    for seed in ss.REPS:
        runs.run(seed, lambda: one(seed))
    runs.done()


# ---- repair --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SWEEP)
def test_repair(gpu, orc, name):
    """t3hip_repair_frame_async (repair_fixed_kernel / repair_generic_kernel: rp_scr_state): both <= t streams come back as the oracle's
    clean stream byte for byte -- header, beacon slots, parity, tail -- with the yardstick's counts (scrambler_seqs.repair_want, held
    against test_repair_semantics.expected on the CPU); a dry run counts the same and stores nothing; the far block is counted and stays."""
    runs = Seeds()

    def one(fr, size):
        tag = (name, size, fr.scr, ss.SEQUENCES[ss.class_of(fr.scr)].kind)
        assert gpu.repair_plan(fr.n_raw, gpu.make_cfg(mode=1, **fr.kw)).path == (1 if name in FUSED else 0)
        clean = fr.clean.reshape(-1)
        for what, s in (("le_t", fr.le_t()), ("tight", fr.tight())):
            exp, words = ss.repair_want(fr, s)
            assert np.array_equal(exp, clean) and words[1] > 0
            got, ver = run_repair(gpu, fr, s, gpu.REPAIR_WRITE)
            assert ver == [0] + words, (tag, what, ver, words)
            assert np.array_equal(got, clean), (tag, what, np.flatnonzero(got != clean)[:8])
        got, ver = run_repair(gpu, fr, s, 0)
        assert ver == [0] + words and np.array_equal(got, s.reshape(-1)), (tag, "dry run", ver)
        s = fr.far()
        exp, words = ss.repair_want(fr, s, [(0, 0)])
        got, ver = run_repair(gpu, fr, s, gpu.REPAIR_WRITE)
        assert ver == [0] + words and np.array_equal(got, exp), (tag, "far", ver, words)

    for size in ss.SIZES:
        seeds = ss.REPS2 if size == "w2" else ss.REPS
        assert ss.classes(seeds) == ALL_CLASSES
        for fr in ss.dec_frames(gpu, name, size, seeds):
            runs.run(fr.scr, lambda: one(fr, size))
    runs.done()


# ---- stages --------------------------------------------------------------------------------------------------------------------------
def test_descramble_stage(gpu, orc):
    """t3hip_descramble_words_dev (the 48-bit replicated tail, the two head bytes), all 81 seeds: 1, 2, 3, 7 and 1000 words at byte offsets
    0 and 2, guard bytes around them; then t3hip_demap_rsdecode_bands_dev on a four-code body descrambled that way."""
    import torch
    assert ss.classes(ss.ALL81) == ALL_CLASSES
    rng = np.random.default_rng(81)
    for n in (1, 2, 3, 7, 1000):
        words = rng.integers(0, 256, 9 * n, dtype=np.uint8)
        for off in (0, 2):
            buf = rng.integers(0, 256, off + 9 * n + 37, dtype=np.uint8); buf[off: off + 9 * n] = words
            for seed in ss.ALL81:
                d = up(buf)
                gpu.descramble_words_dev(d.data_ptr() + off, n, *seed, st())
                torch.cuda.synchronize()
                got = d.cpu().numpy()
                assert np.array_equal(got[:off], buf[:off]) and np.array_equal(got[off + 9 * n:], buf[off + 9 * n:]), (n, off, seed)
                assert np.array_equal(got[off: off + 9 * n], orc.scramble(words, *seed, 1)), (n, off, seed, ss.SEQUENCES[ss.class_of(seed)].kind)
    hdr = gpu.make_cfg(**rp.CONFIGS["four_codes"]); modes = (1, 1, 1, 1); nw = 130
    body = stage_body(orc, rng, hdr, KS, modes, nw, corrupt=1)
    ok, want = restate_stage3(orc, body, hdr, KS, modes)
    assert ok
    total = gpu.demap_rsdecode_bands_syms(nw, hdr, KS)
    for seed in ss.ALL81:
        d = up(orc.scramble(body.reshape(-1), *seed, 0))
        d_out = torch.full((total + 16,), 0xAB, dtype=torch.uint8, device="cuda"); d_nv = torch.zeros(1, dtype=torch.int64, device="cuda")
        gpu.descramble_words_dev(d.data_ptr(), nw, *seed, st())
        assert gpu.demap_rsdecode_bands_dev(d.data_ptr(), nw, hdr, KS, modes, d_out.data_ptr(), total, d_nv.data_ptr(), st()) == total
        torch.cuda.synchronize()
        out = d_out.cpu().numpy()
        assert int(d_nv.item()) == total == len(want) and np.array_equal(out[:total], want) and (out[total:] == 0xAB).all(), seed


# ---- COMPAT decoder ------------------------------------------------------------------------------------------------------------------
COMPAT_SEEDS = [(a, b, s0) for a in range(3) for b in range(3) for s0 in range(3)] + [s.rep for s in ss.SEQUENCES if s.kind == "transient"]


def same_as_oracle(gpu, orc, stream, tag):
    """t3hip_decode_profile and t3hip_decode_frame on a COMPAT stream: ok, the units and cfg_last_seen are the oracle's, whatever they are."""
    oseen = ol.make_cfg(mode=0)
    rc, owords = orc.decode_profile(stream, oseen)
    dctx = gpu.DecoderContext(mode=0)
    ok, words = gpu.decode_profile_to_raw(stream, dctx)
    assert ok == (rc == 0), (tag, ok, rc)
    assert seen_dict(dctx.cfg_last_seen) == seen_dict(oseen), (tag, seen_dict(dctx.cfg_last_seen), seen_dict(oseen))
    if ok:
        assert np.array_equal(fe.u8(words), fe.u8(owords)), (tag, "words")
    oseen = ol.make_cfg(mode=0)
    rc2, opx = orc.decode_frame(stream, oseen)
    dctx = gpu.DecoderContext(mode=0)
    ok2, px = gpu.decode_frame(stream, dctx)
    assert ok2 == (rc2 == 0) and seen_dict(dctx.cfg_last_seen) == seen_dict(oseen), (tag, "frame", ok2, rc2)
    if ok2:
        assert np.array_equal(fe.u8(px), fe.u8(opx)), (tag, "pixels")
    return ok


@pytest.mark.parametrize("name", ("k20", "luma", "k20_beacon83"))
def test_compat_decoder(gpu, orc, name):
    """All 27 (a, b, s0) of {0, 1, 2}^3 and the six transient representatives, whose header carries the seeds mod 27 -- the decoder's
    sequence is then not the encoder's.  On the oracle's COMPAT stream (whose header the reference's decoder refuses: the answer is the
    oracle's, whatever it is), and on a stream laid out as that decoder reads it, scrambled with the sequence of the header's seeds
    (test_oracle_vs_ref.decoder_consistent_stream), clean and with up to two errors in some blocks."""
    rng = np.random.default_rng(zlib.crc32(name.encode()) + 27)
    kw = rp.CONFIGS[name]
    px = rp.rand_pixels(rng, 2161)
    accepted = 0
    for seed in COMPAT_SEEDS:
        ocfg = ol.make_cfg(mode=0, **dict(kw, seed=seed))
        rc, s = orc.encode_frame(px, ocfg); assert rc == 0
        same_as_oracle(gpu, orc, np.ascontiguousarray(s), (name, seed, "encoded"))
        for corrupt in (0, 2):
            s = decoder_consistent_stream(orc, rng, ocfg, 600, corrupt)
            accepted += same_as_oracle(gpu, orc, s, (name, seed, "consistent", corrupt))
    assert accepted >= len(COMPAT_SEEDS)                                          # the clean consistent streams decode
