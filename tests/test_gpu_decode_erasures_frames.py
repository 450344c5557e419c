"""GPU tests of the batched decode with erasures (include/t3hip.h, "decode with erasures of a batch of equal FIXED frames"):
decode_era_frames_px<R, RGB, BCN> -- ONE launch over the tile space of all frames -- for the framings the fused erasure decoder serves,
the loop of the single-frame body for the others, and the synchronous entries.  The yardstick is erasure_patterns.expected_erasures,
proven on the CPU in tests/test_erasure_semantics.py, and the oracle's decoder; what a batch gives for frame f -- output and the four
words -- is what t3hip_decode_erasures_frame_async gives for that frame alone.

Guarding (tests/bounds.py): the coded batch sits in a buffer with NO range that may change, so a written byte of a frame or of a stride
gap fails; the output sits in a buffer whose only ranges that may change are the frames' out_bytes spans; the verdict tensor holds two
spare words behind 4 N that must stay.  Byte work: every comparison is exact."""
import functools

import numpy as np
import pytest

import bounds
import erasure_patterns as ep
import rs_patterns as rp
from test_decode_erasures_plan import FUSED
from test_gpu_decode_erasures import PIXELS, RGB, SIZE, WORDS, _beyond, _frame, _recoverable, expected_pixels, formats, outside, run, want_bytes
from test_gpu_erasure_frames import _kinds, expected_of, layout, round16, stream_of
from test_gpu_erasures import _damage_header

pytestmark = pytest.mark.gpu
FILL = bounds.FILLS[0]
SPARE = 0x07070707                                                        # the two words behind the 4 N verdict words
SEED_B = {"small": 68, "padded": 54}                                      # the second recoverable stream (the first: _recoverable's)
_FAR = {}


def four(w6):
    """the yardstick's six repair words -> the four words of the decode entries"""
    return [0, w6[1], w6[4], w6[5]]


def far_of(orc, fr, case):
    """the refused blocks [(band, block)] of a frame's case, by the yardstick; computed once"""
    key = (fr.name, fr.n_px, case)
    if key not in _FAR:
        _FAR[key] = ep.expected_erasures(orc, fr, stream_of(orc, fr, case))[2]
    return _FAR[key]


@functools.lru_cache(maxsize=16)
def _pixels(name, n_px, case):
    """The pixels a frame's case decodes to outside the tiles of its refused blocks (expected_pixels of test_gpu_decode_erasures.py)"""
    import oracle_lib as ol
    fr = _FRAMES[(name, n_px)]; orc = ol.oracle()
    px = expected_pixels(orc, fr, expected_of(orc, fr, case)[0], far_of(orc, fr, case))
    px.setflags(write=False)
    return px


_FRAMES = {}


def keep_frame(fr):
    _FRAMES[(fr.name, fr.n_px)] = fr
    return fr


def run_batch(gpu, fr, frames, fmt, in_stride=None, out_stride=None, offset=0, fill=FILL, n_frames=None):
    """One t3hip_decode_erasures_frames_async over `frames` (flat byte arrays) -> ([each frame's output bytes], [its four words]).
    The coded batch must come back byte-identical, gaps included; of the output only the frames' spans may change; the two spare
    verdict words must stay."""
    import torch
    cfg = gpu.make_cfg(mode=1, **fr.kw)
    nb, N = len(frames[0]), len(frames) if n_frames is None else n_frames
    p = gpu.decode_erasures_frames_plan(fr.n_raw, len(frames), cfg, fmt)
    units = fr.n_raw if fmt == WORDS else 2 * fr.n_raw
    assert p.frame.in_bytes == nb and p.in_stride_min == nb + (nb & 1) and p.out_bytes == units * SIZE[fmt] and p.out_stride_min == round16(p.out_bytes)
    in_stride = p.in_stride_min if in_stride is None else in_stride
    out_stride = p.out_stride_min if out_stride is None else out_stride
    data, _ = layout(frames, in_stride if len(frames) > 1 else nb)
    inb = bounds.Buf(len(data), fill, offset, data=data, name="coded batch")             # no may_change range: read-only, gaps included
    ob = int(p.out_bytes)
    ostep = out_stride if len(frames) > 1 else ob
    spans = tuple((f * ostep, f * ostep + ob) for f in range(len(frames)))
    out = bounds.Buf(0, fill, 0, data=np.full(spans[-1][1], fill, np.uint8), name="output batch", may_change=spans if N else ())
    ver = torch.full((4 * len(frames) + 2,), SPARE, dtype=torch.int32, device="cuda")
    gpu.decode_erasures_frames_async(inb.ptr, nb // 9, in_stride, N, cfg, fr.n_raw, out.ptr, out_stride, fmt, ver.data_ptr(), torch.cuda.current_stream().cuda_stream)
    bounds.sync()
    inb.result()                                                            # the input byte-identical, its guards intact
    got = out.result()                                                      # guards and gaps intact
    v = ver.cpu().tolist()
    assert v[4 * N:] == [SPARE] * (len(v) - 4 * N), "words behind the batch's verdict words were written"
    return [got[lo:hi] for lo, hi in spans], [v[4 * f: 4 * f + 4] for f in range(len(frames))]


def check_masked(orc, fr, case, got, fmt, tag):
    """A frame's output against the pixels its case decodes to, outside the tiles of its refused blocks"""
    far = far_of(orc, fr, case)
    want = want_bytes(orc, _pixels(fr.name, fr.n_px, case), fmt)
    if not far:
        bounds.check_equal(got, want, FILL, "decoded %s" % (tag,))
        return
    keep = outside(fr, far, fmt)
    assert keep.any() and np.array_equal(got[keep], want[keep]), tag


# ---- 1. the sweep -----------------------------------------------------------------------------------------------------------------------
def recoverable_b(orc, fr, what, not_flagged):
    """The second recoverable stream: admissible pairs only, as _recoverable builds its own, every pair that holds a byte above 26
    followed by one clean block -- or two, or three: the first list whose stream flags another number of blocks than `not_flagged`, by
    the yardstick -> (case for stream_of, flagged blocks)"""
    adm = ep.admissible(max(fr.ks))
    for n_clean in (1, 2, 3):
        only = tuple(x for p in adm if p[0] > 0 for x in (p,) + ("clean",) * n_clean) + tuple(p for p in adm if p[0] == 0)
        case = ("damaged", SEED_B[what], only)
        w = expected_of(orc, fr, case)[1]
        assert w[1] == 0 and far_of(orc, fr, case) == [] and w[4] == w[5] > 0 and (stream_of(orc, fr, case) > 26).any(), (fr.name, what, w)
        if w[4] != not_flagged:
            break
    return case, w[4]


def sweep_streams(orc, name, what):
    """-> (frame, the five streams of the batch, their four words each); asserts on the CPU that A and B differ in their words and both
    hold bytes above 26"""
    fr = keep_frame(_frame(name, what))
    sA, flA = _recoverable(name, what)
    cB, flB = recoverable_b(orc, fr, what, flA)
    sA = np.asarray(sA); sB = stream_of(orc, fr, cB)
    assert flA != flB and (sA > 26).any() and (sB > 26).any() and not np.array_equal(sA, sB), (name, what, flA, flB)
    case = rp.CASES[what][0]
    sC = stream_of(orc, fr, case)
    assert not (sC > 26).any() and four(expected_of(orc, fr, case)[1]) == [0, 0, 0, 0] and four(expected_of(orc, fr, "clean")[1]) == [0, 0, 0, 0]
    wA, wB = [0, 0, flA, flA], [0, 0, flB, flB]
    return fr, [sA, stream_of(orc, fr, "clean"), sC, sB, sA], [wA, [0] * 4, [0] * 4, wB, wA]


@pytest.mark.parametrize("what", ("small", "padded"))
@pytest.mark.parametrize("name", sorted(rp.CONFIGS))
def test_batch_sweep(gpu, orc, name, what):
    """Every framing at two sizes ("small": one tile), every format its decoders produce: recoverable(A), clean, the first case of
    rs_patterns.CASES, recoverable(B), recoverable(A) again, at the smallest strides and at strides with gaps.  Every frame's full output
    is the frame's own pixels; its four words are the yardstick's and those of the single-frame entry on that frame alone."""
    fr, frames, words = sweep_streams(orc, name, what)
    cfg = gpu.make_cfg(mode=1, **fr.kw)
    for fmt in formats(name):
        p = gpu.decode_erasures_frames_plan(fr.n_raw, len(frames), cfg, fmt)
        assert p.one_launch == (1 if name in FUSED and fmt != WORDS else 0) == p.frame.path, (name, fmt)
        want = want_bytes(orc, fr.padded, fmt)
        alone = [run(gpu, fr, s, fmt) for s in frames[:4]] + [None]
        alone[4] = alone[0]
        for in_stride, out_stride in ((None, None), (round16(p.frame.in_bytes) + 32, round16(p.out_bytes) + 32)):
            got, ver = run_batch(gpu, fr, frames, fmt, in_stride, out_stride)
            for f in range(len(frames)):
                tag = (name, what, fmt, in_stride, f)
                assert ver[f] == words[f] == alone[f][1], (tag, ver[f], words[f], alone[f][1])
                bounds.check_equal(got[f], want, FILL, "decoded %s" % (tag,))
                assert np.array_equal(got[f], alone[f][0]), tag


# ---- 2. beyond capacity -----------------------------------------------------------------------------------------------------------------
EVERY_BEYOND = 29


def beyond_streams(orc, name):
    """-> (frame, [(stream, four words, refused blocks, pixels)] of beyond(43), clean, beyond(47)); asserts on the CPU that a quarter of each
    damaged frame's tiles are refused and a quarter are not"""
    fr = keep_frame(_frame(name, "padded"))
    s1, w1, far1, px1 = _beyond(name)
    c2 = ("damaged47", )
    key = (fr.name, fr.n_px, c2)
    if key not in _FAR:
        s2 = ep.damage_frame(orc, fr, 47, every=EVERY_BEYOND)[0]
        e2, w2, far2 = ep.expected_erasures(orc, fr, s2)
        _FAR[key] = (s2, w2, far2, expected_pixels(orc, fr, e2, far2))
    s2, w2, far2, px2 = _FAR[key]
    n_tiles = -(-max(fr.blocks) // 52)
    for w, far in ((w1, far1), (w2, far2)):
        bad = rp.far_tiles_one_k(fr.ks[0], far)
        assert len(bad) >= n_tiles / 4 and n_tiles - len(bad) >= n_tiles / 4, (name, len(bad), n_tiles)
        assert 0 < w[5] < w[4] and w[1] >= w[4] - w[5], (name, w)
    assert not np.array_equal(np.asarray(s1), s2) and far1 != far2
    return fr, [(np.asarray(s1), four(w1), far1, px1), (fr.clean.reshape(-1), [0] * 4, [], fr.padded), (s2, four(w2), far2, px2)]


@pytest.mark.parametrize("name", FUSED)
def test_beyond_capacity(gpu, orc, name):
    """The full damage plan in frames 0 and 2 (two seeds), a clean frame between them: the words are the yardstick's per frame, every
    pixel outside the tiles of the refused blocks is what the yardstick's stream decodes to, and the clean frame is exact with words
    [0, 0, 0, 0] -- the damaged neighbours touch neither."""
    fr, cases = beyond_streams(orc, name)
    cfg = gpu.make_cfg(mode=1, **fr.kw)
    for fmt in (PIXELS, RGB):
        assert gpu.decode_erasures_frames_plan(fr.n_raw, 3, cfg, fmt).one_launch == 1
        got, ver = run_batch(gpu, fr, [c[0] for c in cases], fmt)
        for f, (_, w4, far, px) in enumerate(cases):
            assert ver[f] == w4, (name, fmt, f, ver[f], w4)
            want = want_bytes(orc, px, fmt)
            if not far:
                bounds.check_equal(got[f], want, FILL, "the clean frame between damaged ones, %s fmt %d" % (name, fmt))
            else:
                keep = outside(fr, far, fmt)
                assert keep.any() and np.array_equal(got[f][keep], want[keep]), (name, fmt, f)


# ---- 3. the generic path ----------------------------------------------------------------------------------------------------------------
def test_generic_path(gpu, orc):
    """four_codes (the loop of the single-frame body): the words of each frame, pixels and raw words."""
    fr = keep_frame(_frame("four_codes", "padded"))
    s, w, far, _ = _beyond("four_codes")
    assert 0 < w[5] < w[4] and w[1] > 0
    frames = [np.asarray(s), fr.clean.reshape(-1), np.asarray(s)]
    for fmt in (PIXELS, WORDS):
        assert gpu.decode_erasures_frames_plan(fr.n_raw, 3, gpu.make_cfg(mode=1, **fr.kw), fmt).one_launch == 0
        got, ver = run_batch(gpu, fr, frames, fmt)
        assert ver == [four(w), [0] * 4, four(w)], (fmt, ver, w)
        bounds.check_equal(got[1], want_bytes(orc, fr.padded, fmt), FILL, "the clean frame of the generic batch, fmt %d" % fmt)


# ---- 4. the header word -----------------------------------------------------------------------------------------------------------------
def test_header_word(gpu, orc):
    """One header symbol of frame 1 changed; in another run a header byte of frame 2 set to 0xFF: only that frame's word 4 f is 1, and
    all outputs are still the frames' pixels."""
    fr, frames, words = sweep_streams(orc, "k20", "padded")
    want = want_bytes(orc, fr.padded, PIXELS)
    for f_bad, at, value in ((1, 5, None), (2, 40, 0xFF)):
        fs = [s.copy() for s in frames[:4]]
        fs[f_bad][at] = (fs[f_bad][at] + 1) % 27 if value is None else value
        got, ver = run_batch(gpu, fr, fs, PIXELS)
        for f in range(4):
            assert ver[f] == [1 if f == f_bad else 0] + words[f][1:], (f_bad, f, ver[f])
            bounds.check_equal(got[f], want, FILL, "header word run %d, frame %d" % (f_bad, f))


# ---- 5. addresses -----------------------------------------------------------------------------------------------------------------------
def _small_odd(gpu, orc, name):
    """A frame of a few ragged tiles whose coded word count is odd, so that its byte count is, and in_bytes + 1 no multiple of 16"""
    cfg = gpu.make_cfg(mode=1, **rp.CONFIGS[name])
    n_px = 3 * 2160 + 301
    while int(gpu.plan((n_px + 1) // 2, cfg).out_words) % 2 != 1 or (9 * int(gpu.plan((n_px + 1) // 2, cfg).out_words) + 1) % 16 == 0:
        n_px += 2
    return keep_frame(rp.Frame(orc, lambda n_raw: gpu.plan(n_raw, cfg), name, n_px, 105))


def address_cases(orc, fr):
    """recoverable A, far1 (tile 0 refused, no flagged byte), clean, recoverable B: all but one frame are compared in full"""
    adm = ep.admissible(fr.ks[0])
    A = ("damaged", 71, tuple(adm + ["sched", "clean"]))
    B = ("damaged", 72, tuple(x for p in adm if p[0] > 0 for x in (p, "clean")) + tuple(p for p in adm if p[0] == 0))
    wa, wb = expected_of(orc, fr, A)[1], expected_of(orc, fr, B)[1]
    assert wa[1] == wb[1] == 0 and wa[4] == wa[5] > 0 and wb[4] == wb[5] > 0 and wa[4] != wb[4], (fr.name, wa, wb)
    assert (stream_of(orc, fr, A) > 26).any() and (stream_of(orc, fr, B) > 26).any()
    assert rp.far_tiles_one_k(fr.ks[0], far_of(orc, fr, "far1")) == [0] and not (stream_of(orc, fr, "far1") > 26).any()
    return [A, "far1", "clean", B]


@pytest.mark.parametrize("name", ("k20", "k20_beacon83"))
def test_addresses(gpu, orc, name):
    """Base at 2 mod 16 and frames of an odd byte count in_bytes + 1 apart: every frame but the first starts off every 4-byte boundary
    -- the byte-wise header compare, load16 and the aligned dwords of load_run<true> --, over both fills."""
    fr = _small_odd(gpu, orc, name)
    cases = address_cases(orc, fr)
    p = gpu.decode_erasures_frames_plan(fr.n_raw, len(cases), gpu.make_cfg(mode=1, **fr.kw), PIXELS)
    assert p.frame.in_bytes % 2 == 1 and p.in_stride_min == p.frame.in_bytes + 1 and p.one_launch == 1 and p.frame.n_tiles > 1
    assert len({(2 + f * p.in_stride_min) % 16 for f in range(len(cases))}) > 1                 # the frames start at different offsets inside a 16-byte granule
    for fill in bounds.FILLS:
        got, ver = run_batch(gpu, fr, [stream_of(orc, fr, c) for c in cases], PIXELS, in_stride=p.frame.in_bytes + 1, offset=2, fill=fill)
        for f, c in enumerate(cases):
            assert ver[f] == four(expected_of(orc, fr, c)[1]), (name, fill, f, c, ver[f])
            check_masked(orc, fr, c, got[f], PIXELS, (name, fill, f, c))


# ---- 6. frame crossing ------------------------------------------------------------------------------------------------------------------
def crossing_cases(orc, fr):
    """damaged A, far2 (no flagged byte), damaged B, clean; asserts that the damaged streams hold flagged blocks in tile 0 and in tile 6"""
    A, B = ("damaged", 61), ("damaged", 62)
    wa, wb = expected_of(orc, fr, A)[1], expected_of(orc, fr, B)[1]
    assert 0 < wa[5] < wa[4] and 0 < wb[5] < wb[4] and wa != wb, (fr.name, wa, wb)
    f0 = rp.band_first_block(fr.L); Bi = rp.block_index(fr.L, fr.ocfg)
    for c in (A, B):
        planned = ep.damage_frame(orc, fr, c[1], only=_kinds(fr, c[1]))[1]
        hi = (stream_of(orc, fr, c)[Bi] > 26).any(axis=1)
        flagged = np.concatenate([np.flatnonzero((hi & planned)[f0[b]: f0[b] + fr.blocks[b]]) // 52 for b in range(9)])
        assert {0, 6} <= set(flagged.tolist()), (c, sorted(set(flagged.tolist())))
    assert not (stream_of(orc, fr, "far2") > 26).any() and expected_of(orc, fr, "far2")[1][1] == 2
    return (A, "far2", B, "clean")


@pytest.mark.parametrize("name", ("k20", "k20_beacon83"))
def test_frame_crossing(gpu, orc, name):
    """Frames of 7 tiles, the last ragged and the pixel count odd, so many of them that every workgroup (two per CU) draws more than two
    tickets and changes frame off the grid's rhythm; four streams cycled over the frames.  Per-frame words are exact, and so are the sums
    over the frames of words 1 to 3 -- a lost or doubled flush at a frame change and a wrong frame base show; bytes outside the refused
    tiles are exact."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n_frames = -(-(9 * cus + 1) // 7)
    cfg = gpu.make_cfg(mode=1, **rp.CONFIGS[name])
    fr = keep_frame(rp.Frame(orc, lambda n_raw: gpu.plan(n_raw, cfg), name, 7 * 2160 - 1001, 104))
    p = gpu.decode_erasures_frames_plan(fr.n_raw, n_frames, cfg, PIXELS)
    assert p.one_launch == 1 and p.frame.n_tiles == 7 and n_frames * 7 >= 9 * cus + 1
    cycle = crossing_cases(orc, fr)
    cases = [cycle[f % 4] for f in range(n_frames)]
    got, ver = run_batch(gpu, fr, [stream_of(orc, fr, c) for c in cases], PIXELS)
    want4 = {c: four(expected_of(orc, fr, c)[1]) for c in cycle}
    wrong = [(f, cases[f], ver[f], want4[cases[f]]) for f in range(n_frames) if ver[f] != want4[cases[f]]]
    assert not wrong, (len(wrong), wrong[:4])
    for i in (1, 2, 3):
        assert sum(v[i] for v in ver) == sum(want4[c][i] for c in cases), ("word", i)
    masks = {c: (outside(fr, far_of(orc, fr, c), PIXELS) if far_of(orc, fr, c) else None) for c in cycle}
    wants = {c: want_bytes(orc, _pixels(fr.name, fr.n_px, c), PIXELS) for c in cycle}
    for f, c in enumerate(cases):
        keep = masks[c]
        ok = np.array_equal(got[f], wants[c]) if keep is None else np.array_equal(got[f][keep], wants[c][keep])
        assert ok, (name, "frame", f, c)


# ---- 7. n_frames 0 and 1 ----------------------------------------------------------------------------------------------------------------
def test_zero_and_one_frame(gpu, orc):
    """n_frames = 0 launches and writes nothing -- the verdict keeps its fill, the output its own; n_frames = 1 is the single-frame entry,
    whatever the stride arguments say (0 here)."""
    fr, frames, words = sweep_streams(orc, "k20", "small")
    for fmt in (PIXELS, WORDS):
        got, ver = run_batch(gpu, fr, frames[:2], fmt, n_frames=0)
        assert all((g == FILL).all() for g in got) and ver == [[SPARE] * 4] * 2, (fmt, ver)
        alone, w = run(gpu, fr, frames[0], fmt)
        got, ver = run_batch(gpu, fr, frames[:1], fmt, in_stride=0, out_stride=0)
        assert ver == [w] == [words[0]] and np.array_equal(got[0], alone), (fmt, ver, w)
        bounds.check_equal(got[0], want_bytes(orc, fr.padded, fmt), FILL, "one frame, fmt %d" % fmt)


# ---- 8. the synchronous entries ---------------------------------------------------------------------------------------------------------
def sync_batch(gpu, orc, fr):
    """clean | 2 header errors + recoverable | header beyond t | mixed | clean -> (frames, the case each body is, frame_rc, four counts)"""
    within = ("damaged", 35, tuple(ep.admissible(fr.ks[0])))
    mixed = ("damaged", 36)
    s_within, s_mixed, clean = stream_of(orc, fr, within), stream_of(orc, fr, mixed), stream_of(orc, fr, "clean")
    w_within, w_mixed = expected_of(orc, fr, within)[1], expected_of(orc, fr, mixed)[1]
    assert w_within[1] == 0 and w_within[5] == w_within[4] > 0 and w_mixed[1] > 0 and 0 < w_mixed[5] < w_mixed[4]
    frames = [clean, _damage_header(s_within, 2), _damage_header(s_within, 9), s_mixed, clean]
    counts = [[0] * 4, four(w_within), [0] * 4, four(w_mixed), [0] * 4]
    return frames, ["clean", within, None, mixed, "clean"], [gpu.OK, gpu.OK, gpu.E_HEADER, gpu.E_RS, gpu.OK], counts


def test_synchronous_entries(gpu, orc):
    """The _dev and the host form at two strides: the frame whose header does not decode reports E_HEADER and zero counts, its output
    span is untouched, and it splits the batch into two runs; counts[4 f] is 0 although frame 1's header holds two errors; the input
    buffer and the host input array are unchanged.  No decodable header: E_HEADER, nothing written.  cap_units one short: E_CAPACITY
    for the frames, nothing written, the call itself T3_OK with the units one frame needs."""
    import torch
    fr = keep_frame(_frame("k20", "padded"))
    frames, cases, want_rc, want_counts = sync_batch(gpu, orc, fr)
    nb, N, units = len(frames[0]), len(frames), 2 * fr.n_raw
    ob = 6 * units
    st = torch.cuda.current_stream().cuda_stream
    for in_stride, out_stride in ((nb + (nb & 1), round16(ob)), (round16(nb) + 32, round16(ob) + 32)):
        data, _ = layout(frames, in_stride)
        spans = tuple((f * out_stride, f * out_stride + ob) for f in range(N))
        inb = bounds.Buf(len(data), FILL, 2, data=data, name="coded batch")
        out = bounds.Buf(0, FILL, 0, data=np.full(spans[-1][1], FILL, np.uint8), name="output batch", may_change=[spans[f] for f in range(N) if cases[f] is not None])
        seen = gpu.DecoderContext(mode=1).cfg_last_seen
        rc, n, rcs, counts = gpu.decode_erasures_frames_dev(inb.ptr, nb // 9, in_stride, N, seen, out.ptr, out_stride, units, PIXELS, st)
        bounds.sync()
        assert rc == gpu.OK and n == units and rcs == want_rc and counts == want_counts, (in_stride, rc, n, rcs, counts)
        assert seen.profile == rp.CONFIGS["k20"]["profile"] and seen.mode == 1
        inb.result()
        got = out.result()                                                  # the E_HEADER frame's span is no may_change range: untouched
        for f, c in enumerate(cases):
            if c is not None:
                check_masked(orc, fr, c, got[spans[f][0]: spans[f][1]], PIXELS, ("dev", in_stride, f))
        # the host form: rows of in_stride bytes, the pad behind a frame is neither read nor written
        w, _ = layout(frames, in_stride)
        w = np.concatenate([w, np.full(in_stride - nb, 0x3C, np.uint8)]).reshape(N, in_stride)
        before = w.copy()
        ctx = gpu.DecoderContext(mode=1)
        rc, rcs, outs, counts = gpu.decode_erasures_frames(w, ctx, PIXELS)
        assert rc == gpu.OK and rcs == want_rc and counts == want_counts and np.array_equal(w, before), (in_stride, "host", rc, rcs, counts)
        assert ctx.cfg_last_seen.profile == rp.CONFIGS["k20"]["profile"]
        for f, c in enumerate(cases):
            if c is None:
                assert outs[f].size == 0
            else:
                check_masked(orc, fr, c, np.ascontiguousarray(outs[f]).view(np.uint8).reshape(-1), PIXELS, ("host", in_stride, f))
    # the host entry itself: a refused frame's span of the caller's output array stays as it was
    import ctypes as C
    flat, _ = layout(frames, nb + (nb & 1))
    hout = np.full(N * ob, 0xEE, np.uint8); cnt = (C.c_uint32 * (4 * N))(); rcs = (C.c_int * N)(); n = C.c_uint64()
    ctx = gpu.DecoderContext(mode=1)
    rc = gpu.lib().t3hip_decode_erasures_frames(flat.ctypes.data_as(C.c_void_p), C.c_uint64(nb // 9), C.c_uint64(nb + (nb & 1)), C.c_uint32(N), C.byref(ctx.cfg_last_seen),
                                                hout.ctypes.data_as(C.c_void_p), C.c_uint64(ob), C.c_uint64(units), C.byref(n), C.c_int(PIXELS), cnt, rcs)
    assert rc == gpu.OK and list(rcs) == want_rc and n.value == units and (hout[2 * ob: 3 * ob] == 0xEE).all()
    bounds.check_equal(hout[4 * ob:], want_bytes(orc, fr.padded, PIXELS), 0xEE, "host entry, last frame")
    # no header decodes: E_HEADER, nothing written
    bad = [_damage_header(frames[0], 9)] * 2
    data, _ = layout(bad, nb + (nb & 1))
    inb = bounds.Buf(len(data), FILL, 0, data=data, name="coded batch"); out = bounds.Buf(round16(ob) + ob, FILL, 0, name="output batch")
    rc, n, rcs, counts = gpu.decode_erasures_frames_dev(inb.ptr, nb // 9, nb + (nb & 1), 2, gpu.DecoderContext(mode=1).cfg_last_seen, out.ptr, round16(ob), units, PIXELS, st)
    bounds.sync()
    assert rc == gpu.E_HEADER and n == 0 and rcs == [gpu.E_HEADER] * 2 and counts == [[0] * 4] * 2
    inb.result(); out.untouched()
    rc, rcs, outs, counts = gpu.decode_erasures_frames(np.stack(bad), gpu.DecoderContext(mode=1), PIXELS)
    assert rc == gpu.E_HEADER and rcs == [gpu.E_HEADER] * 2 and counts == [[0] * 4] * 2 and all(o.size == 0 for o in outs)
    # seen->mode must be FIXED on entry
    with pytest.raises(gpu.T3Error) as e:
        gpu.decode_erasures_frames(np.stack(frames), gpu.DecoderContext(mode=0), PIXELS)
    assert e.value.code == gpu.E_ARG
    # one unit short: the frames whose header decodes report E_CAPACITY, nothing is written, the call says what a frame needs
    data, _ = layout(frames, nb + (nb & 1))
    inb = bounds.Buf(len(data), FILL, 0, data=data, name="coded batch"); out = bounds.Buf((N - 1) * round16(ob) + ob, FILL, 0, name="output batch")
    rc, n, rcs, counts = gpu.decode_erasures_frames_dev(inb.ptr, nb // 9, nb + (nb & 1), N, gpu.DecoderContext(mode=1).cfg_last_seen, out.ptr, round16(ob), units - 1, PIXELS, st)
    bounds.sync()
    assert rc == gpu.OK and n == units and rcs == [gpu.E_CAPACITY if c is not None else gpu.E_HEADER for c in cases] and counts == [[0] * 4] * N, (rc, n, rcs)
    inb.result(); out.untouched()


# ---- 9. two configurations in one batch -------------------------------------------------------------------------------------------------
def test_two_configurations_in_one_batch(gpu, orc):
    """A A B B A: five frames of one profile and one n_raw_words whose scrambler seeds differ, pixels, through the _dev and the host
    entry.  The runs are 2, 2, 1 -- the one launch twice and the single-frame body inside a batch -- and every frame's pixels (outside
    the tiles of its refused blocks), counts and code are the yardstick's for that frame alone.  (The yardsticks are computed here, not
    through this file's caches: those are keyed by a frame's name and size, which A and B share.)"""
    import torch
    from test_gpu_repair_frames import two_configurations
    A, B = two_configurations(gpu, orc, _small_odd(gpu, orc, "k20").n_px)
    order = (A, A, B, B, A)
    cfg = gpu.make_cfg(mode=1, **A.kw)
    p = gpu.decode_erasures_frames_plan(A.n_raw, 2, cfg, PIXELS)
    assert p.one_launch == 1 and p.frame.path == 1 and p.frame.n_tiles >= 2
    adm = list(ep.admissible(A.ks[0]))
    received = [ep.damage_frame(orc, A, 91, only=adm)[0], A.clean.reshape(-1), ep.damage_frame(orc, B, 92, only=_kinds(B, 92))[0], ep.damage_frame(orc, B, 93, only=adm)[0], None]
    received[4] = received[0]
    frames = [np.ascontiguousarray(s, np.uint8).reshape(-1) for s in received]
    yard = [ep.expected_erasures(orc, fr, s) for fr, s in zip(order, frames)]
    want_counts = [four(w) for _, w, _ in yard]
    want_rc = [gpu.E_RS if c[1] else gpu.OK for c in want_counts]
    assert gpu.OK in want_rc and want_counts[0][2] > 0 and want_counts[2] != want_counts[0] and want_counts[1] == [0] * 4, (want_rc, want_counts)
    want = [want_bytes(orc, expected_pixels(orc, fr, e, far), PIXELS) for fr, (e, _, far) in zip(order, yard)]
    keep = [outside(fr, far, PIXELS) if far else None for fr, (_, _, far) in zip(order, yard)]

    def check(got, f, tag):
        if keep[f] is None:
            bounds.check_equal(got, want[f], FILL, "two configurations %s, frame %d" % (tag, f))
        else:
            assert keep[f].any() and np.array_equal(got[keep[f]], want[f][keep[f]]), (tag, f)

    nb, N, units = len(frames[0]), len(frames), 2 * A.n_raw
    ob = 6 * units
    in_stride, out_stride = nb + (nb & 1), round16(ob)
    data, _ = layout(frames, in_stride)
    spans = tuple((f * out_stride, f * out_stride + ob) for f in range(N))
    inb = bounds.Buf(len(data), FILL, 2, data=data, name="coded batch")
    out = bounds.Buf(0, FILL, 0, data=np.full(spans[-1][1], FILL, np.uint8), name="output batch", may_change=spans)
    seen = gpu.DecoderContext(mode=1).cfg_last_seen
    rc, n, rcs, counts = gpu.decode_erasures_frames_dev(inb.ptr, nb // 9, in_stride, N, seen, out.ptr, out_stride, units, PIXELS, torch.cuda.current_stream().cuda_stream)
    bounds.sync()
    assert rc == gpu.OK and n == units and rcs == want_rc and counts == want_counts, (rc, n, rcs, counts, want_counts)
    inb.result()
    got = out.result()
    for f, (lo, hi) in enumerate(spans):
        check(got[lo:hi], f, "dev")
    w, _ = layout(frames, in_stride)
    w = np.concatenate([w, np.full(in_stride - nb, 0x3C, np.uint8)]).reshape(N, in_stride)
    before = w.copy()
    rc, rcs, outs, counts = gpu.decode_erasures_frames(w, gpu.DecoderContext(mode=1), PIXELS)
    assert rc == gpu.OK and rcs == want_rc and counts == want_counts and np.array_equal(w, before), ("host", rc, rcs, counts)
    for f in range(N):
        check(np.ascontiguousarray(outs[f]).view(np.uint8).reshape(-1), f, "host")
