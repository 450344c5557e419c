"""GPU tests of the batched repair with erasures (include/t3hip.h, "repair with erasures of a batch of equal FIXED frames"):
erasure_frames_kernel<R> -- ONE launch over the tile space of all frames -- for the framings the fused kernel serves, the loop of the
single-frame erasure body for the others, and the synchronous entries.  The yardstick is erasure_patterns.expected_erasures, proven on
the CPU in tests/test_erasure_semantics.py; what a batch does to frame f -- bytes and the six words -- is what
t3hip_repair_erasures_frame_async does to that frame alone.  One guarded buffer per batch (tests/bounds.py): the frames' bytes may
change, the gaps of a stride and the guards may not; the verdict tensor holds two spare words behind 6 N that must stay.  Byte work:
every comparison is exact.

Streams: erasure_patterns.damage_frame with distinct seeds.  At "small" (301 pixels, 7 to 9 blocks a band) the default plan of kinds does
not reach a beyond-capacity block in every configuration and gives the same words for every seed, so there the kinds are
admissible(k) + beyond(k) of the frame's first band, rotated by the seed (`only=`): every damaged stream then holds accepted and refused
flagged blocks, and two seeds differ -- the tests assert both."""
import json
import os
import subprocess

import numpy as np
import pytest

import bounds
import erasure_patterns as ep
import rs_patterns as rp
from test_gpu_erasures import _damage_header, _frame, run as run_single
from test_repair_semantics import FUSED, GENERIC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = bounds.FILLS[0]
GAP = 0x3C                                                                # what the bytes of a stride behind a frame hold
SPARE = 0x07070707                                                        # the two words behind the 6 N verdict words
SWEEP = FUSED + GENERIC
SEEDS = {"small": (51, 68), "padded": (53, 54)}                           # seeds A and B of the damaged streams
_STREAMS, _EXPECTED = {}, {}


def _kinds(fr, seed):
    """None (damage_frame's own plan) for a frame whose bands hold it; for a frame of a few blocks a band the admissible and the
    beyond-capacity pairs of its first band's code, rotated by the seed"""
    if min(fr.blocks) > 2 * len(ep.frame_kinds(min(fr.ks))):
        return None
    kinds = ep.admissible(fr.ks[0]) + ep.beyond(fr.ks[0])
    r = seed % len(kinds)
    return kinds[r:] + kinds[:r]


def stream_of(orc, fr, case):
    """The received stream (flat, read-only) of a frame's case, built once: 'clean', a case of rs_patterns.CASES (no byte above 26), or
    ('damaged', seed[, only]) -- erasure_patterns.damage_frame"""
    key = (fr.name, fr.n_px, case)
    if key not in _STREAMS:
        if case == "clean":
            s = fr.clean
        elif isinstance(case, tuple):
            s = ep.damage_frame(orc, fr, case[1], only=list(case[2]) if len(case) > 2 else _kinds(fr, case[1]))[0]
        else:
            s = fr.stream(case)[0]
        s = np.ascontiguousarray(s, np.uint8).reshape(-1).copy()
        s.setflags(write=False)
        _STREAMS[key] = s
    return _STREAMS[key]


def expected_of(orc, fr, case):
    """The yardstick's (R', six words) of a frame's case, computed once and never changed"""
    key = (fr.name, fr.n_px, case)
    if key not in _EXPECTED:
        e, w, _ = ep.expected_erasures(orc, fr, stream_of(orc, fr, case))
        e.setflags(write=False)
        _EXPECTED[key] = (e, w)
    return _EXPECTED[key]


def round16(x):
    return (x + 15) & ~15


def layout(frames, stride):
    nb, N = len(frames[0]), len(frames)
    data = np.full((N - 1) * stride + nb, GAP, np.uint8)
    for f, s in enumerate(frames):
        data[f * stride: f * stride + nb] = s
    return data, tuple((f * stride, f * stride + nb) for f in range(N))


def run_batch(gpu, fr, frames, flags, stride=None, offset=0, fill=FILL, era=True):
    """One t3hip_repair_erasures_frames_async (era=False: t3hip_repair_frames_async) over `frames` (flat byte arrays) in one guarded
    buffer -> ([each frame's bytes afterwards], [its six (four) words]); guards, gaps and the two spare words are checked, every byte of
    a frame may change."""
    import torch
    cfg = gpu.make_cfg(mode=1, **fr.kw)
    nb, N, nw = len(frames[0]), len(frames), 6 if era else 4
    p = gpu.repair_frames_plan(fr.n_raw, N, cfg)
    assert p.in_bytes == nb and p.stride_min == nb + (nb & 1)
    stride = p.stride_min if stride is None else stride
    data, spans = layout(frames, stride)
    buf = bounds.Buf(len(data), fill, offset, data=data, name="batch", may_change=spans)
    ver = torch.full((nw * N + 2,), SPARE, dtype=torch.int32, device="cuda")
    fn = gpu.repair_erasures_frames_async if era else gpu.repair_frames_async
    fn(buf.ptr, nb // 9, stride, N, cfg, fr.n_raw, flags, ver.data_ptr(), torch.cuda.current_stream().cuda_stream)
    bounds.sync()
    got = buf.result()
    v = ver.cpu().tolist()
    assert v[nw * N:] == [SPARE] * 2, "words behind the batch's verdict words were written"
    return [got[lo:hi] for lo, hi in spans], [v[nw * f: nw * f + nw] for f in range(N)]


def check_batch(gpu, orc, fr, cases, tag, **kw):
    """A batch of a frame's cases under T3_REPAIR_WRITE against the yardstick -> (bytes, words) per frame"""
    got, ver = run_batch(gpu, fr, [stream_of(orc, fr, c) for c in cases], gpu.REPAIR_WRITE, **kw)
    for f, c in enumerate(cases):
        exp, words = expected_of(orc, fr, c)
        assert ver[f] == words, (tag, f, c, "words", ver[f], words)
        bounds.check_equal(got[f], exp, kw.get("fill", FILL), "repaired %s frame %d (%s)" % (tag, f, c))
    return got, ver


def assert_bite(orc, fr, a, b):
    """Damaged streams a and b hold accepted and refused flagged blocks, and differ in their words"""
    wa, wb = expected_of(orc, fr, a)[1], expected_of(orc, fr, b)[1]
    assert 0 < wa[5] < wa[4] and 0 < wb[5] < wb[4] and wa != wb, (fr.name, wa, wb)
    assert (stream_of(orc, fr, a) > 26).any() and (stream_of(orc, fr, b) > 26).any()


# ---- 1. the main sweep ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ("small", "padded"))
@pytest.mark.parametrize("name", SWEEP)
def test_batch_sweep(gpu, orc, name, what):
    """Every framing at two sizes: damaged(A), clean, the first case of rs_patterns.CASES, damaged(B), damaged(A) again, at the smallest
    stride and at a 16-byte one with gaps; bytes and six words are the yardstick's and those of the single-frame entry on each frame
    alone."""
    fr = _frame(name, what)
    A, B = (("damaged", s) for s in SEEDS[what])
    cases = [A, "clean", rp.CASES[what][0], B, A]
    assert_bite(orc, fr, A, B)
    p = gpu.repair_frames_plan(fr.n_raw, len(cases), gpu.make_cfg(mode=1, **fr.kw))
    assert p.one_launch == (1 if name in FUSED else 0) and p.path == p.one_launch
    alone = {c: run_single(gpu, fr, stream_of(orc, fr, c), gpu.REPAIR_WRITE) for c in set(cases)}
    for stride in (p.stride_min, round16(p.in_bytes) + 32):
        got, ver = check_batch(gpu, orc, fr, cases, (name, what, stride), stride=stride)
        for f, c in enumerate(cases):
            assert ver[f] == alone[c][1] and np.array_equal(got[f], alone[c][0]), (name, what, stride, f, c, "single-frame entry")
    assert expected_of(orc, fr, "clean")[1] == [0] * 6 and not (stream_of(orc, fr, cases[2]) > 26).any()


# ---- 2. dry run, second repair ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("k20", "k20_beacon83"))
def test_dry_run_and_second_repair(gpu, orc, name):
    """Without T3_REPAIR_WRITE: the same words, the buffer unchanged.  A repair of the repaired batch: [0, w1, 0, 0, w4 - w5, 0] per
    frame, nothing written."""
    fr = _frame(name, "padded")
    A, B = (("damaged", s) for s in SEEDS["padded"])
    cases = [A, "clean", "sched", B, A]
    frames = [stream_of(orc, fr, c) for c in cases]
    got, ver = run_batch(gpu, fr, frames, 0)
    for f, c in enumerate(cases):
        assert ver[f] == expected_of(orc, fr, c)[1], (name, f, c, "dry run", ver[f])
        assert np.array_equal(got[f], frames[f]), (name, f, c, "dry run wrote")
    repaired = [expected_of(orc, fr, c)[0] for c in cases]
    got, ver = run_batch(gpu, fr, repaired, gpu.REPAIR_WRITE)
    for f, c in enumerate(cases):
        w = expected_of(orc, fr, c)[1]
        assert ver[f] == [0, w[1], 0, 0, w[4] - w[5], 0], (name, f, c, "second repair", ver[f])
        assert np.array_equal(got[f], repaired[f]), (name, f, c, "second repair wrote")


# ---- 3. isolation -----------------------------------------------------------------------------------------------------------------------
def test_isolation(gpu, orc):
    """clean, damaged, clean: the damaged frame changes neither its neighbours' words nor their bytes."""
    fr = _frame("k20", "padded")
    D = ("damaged", SEEDS["padded"][0])
    got, ver = check_batch(gpu, orc, fr, ["clean", D, "clean"], "isolation")
    clean = stream_of(orc, fr, "clean")
    assert ver[0] == ver[2] == [0] * 6 and np.array_equal(got[0], clean) and np.array_equal(got[2], clean)
    assert ver[1][1] > 0 and ver[1][2] > 0 and ver[1][5] > 0


# ---- 4. the header word -----------------------------------------------------------------------------------------------------------------
def test_header_word(gpu, orc):
    """One symbol of frame 1's header changed: its word 0 is 1, every other frame's 0; all bodies are repaired, no header is touched."""
    fr = _frame("k20", "padded")
    A, B = (("damaged", s) for s in SEEDS["padded"])
    cases = [A, A, B, "clean"]
    frames = [stream_of(orc, fr, c).copy() for c in cases]
    frames[1][5] = (frames[1][5] + 1) % 27
    got, ver = run_batch(gpu, fr, frames, gpu.REPAIR_WRITE)
    hs = int(fr.L.header_syms)
    for f, c in enumerate(cases):
        exp, words = expected_of(orc, fr, c)
        want = exp.copy(); want[:hs] = frames[f][:hs]
        assert ver[f] == [1 if f == 1 else 0] + words[1:], (f, c, ver[f])
        bounds.check_equal(got[f], want, FILL, "header word, frame %d" % f)


# ---- 5. addresses -----------------------------------------------------------------------------------------------------------------------
def _small_k20(gpu, orc, odd_words):
    """A k20 frame of a few ragged tiles whose coded word count is odd (so that 9 * words is) or even"""
    cfg = gpu.make_cfg(mode=1, **rp.CONFIGS["k20"])
    n_px = 3 * 2160 + 301
    while int(gpu.plan((n_px + 1) // 2, cfg).out_words) % 2 != (1 if odd_words else 0):
        n_px += 2
    return rp.Frame(orc, lambda n_raw: gpu.plan(n_raw, cfg), "k20", n_px, 105)


def test_addresses(gpu, orc):
    """Base at 2 mod 16 and frames of an odd byte count stride_min = in_bytes + 1 apart: every frame but the first starts off every
    16-byte boundary; over both fills."""
    fr = _small_k20(gpu, orc, True)
    p = gpu.repair_frames_plan(fr.n_raw, 4, gpu.make_cfg(mode=1, **fr.kw))
    assert p.in_bytes % 2 == 1 and p.stride_min == p.in_bytes + 1 and p.one_launch == 1 and p.tiles_per_frame > 1
    A, B = ("damaged", 71), ("damaged", 72)
    assert_bite(orc, fr, A, B)
    for fill in bounds.FILLS:
        check_batch(gpu, orc, fr, [A, "far1", "clean", B], ("addresses", fill), offset=2, fill=fill)


# ---- 6. frame crossing ------------------------------------------------------------------------------------------------------------------
def test_frame_crossing(gpu, orc):
    """Frames of 7 tiles, the last ragged and the pixel count odd, so many of them that every workgroup walks more than two tiles and
    changes frame at points that do not line up with the grid; four streams cycled over the frames.  Every frame's bytes and six words
    are the yardstick's: the per-frame sums of words 1 to 5 are exact, so a lost or doubled flush at a frame change and a wrong frame
    base show.  The damaged streams hold flagged blocks in tile 0 and in tile 6."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n_frames = -(-(9 * cus + 1) // 7)
    cfg = gpu.make_cfg(mode=1, **rp.CONFIGS["k20"])
    fr = rp.Frame(orc, lambda n_raw: gpu.plan(n_raw, cfg), "k20", 7 * 2160 - 1001, 104)
    p = gpu.repair_frames_plan(fr.n_raw, n_frames, cfg)
    assert p.one_launch == 1 and p.tiles_per_frame == 7 and n_frames * 7 >= 9 * cus + 1
    A, B = ("damaged", 61), ("damaged", 62)
    assert_bite(orc, fr, A, B)
    f0 = rp.band_first_block(fr.L)
    for c in (A, B):
        planned = ep.damage_frame(orc, fr, c[1])[1]
        tiles = np.concatenate([np.flatnonzero(planned[f0[b]: f0[b] + fr.blocks[b]]) // 52 for b in range(9)])
        Bi = rp.block_index(fr.L, fr.ocfg)
        hi = (stream_of(orc, fr, c)[Bi] > 26).any(axis=1)
        flagged = np.concatenate([np.flatnonzero((hi & planned)[f0[b]: f0[b] + fr.blocks[b]]) // 52 for b in range(9)])
        assert {0, 6} <= set(tiles.tolist()) and {0, 6} <= set(flagged.tolist()), (c, sorted(set(flagged.tolist())))
    assert not (stream_of(orc, fr, "far2") > 26).any() and expected_of(orc, fr, "far2")[1][1] == 2
    cycle = (A, "far2", B, "clean")
    cases = [cycle[f % 4] for f in range(n_frames)]
    got, ver = check_batch(gpu, orc, fr, cases, "crossing")
    for i in range(1, 6):
        assert sum(v[i] for v in ver) == sum(expected_of(orc, fr, c)[1][i] for c in cases), ("word", i)


# ---- 7. no flagged byte: the plain batch ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SWEEP)
def test_without_flagged_bytes_is_the_plain_batch(gpu, orc, name):
    """On the streams of rs_patterns.CASES (no byte above 26) plus a clean frame, bytes and words [0..3] are t3hip_repair_frames_async's
    on the same batch, [4] = [5] = 0."""
    fr = _frame(name, "small")
    cases = list(rp.CASES["small"]) + ["clean"]
    frames = [stream_of(orc, fr, c) for c in cases]
    assert not any((s > 26).any() for s in frames)
    want, w4 = run_batch(gpu, fr, frames, gpu.REPAIR_WRITE, era=False)
    got, w6 = run_batch(gpu, fr, frames, gpu.REPAIR_WRITE)
    for f, c in enumerate(cases):
        assert w6[f] == w4[f] + [0, 0], (name, f, c, w6[f], w4[f])
        assert np.array_equal(got[f], want[f]), (name, f, c)
    assert w6[-1] == [0] * 6 and np.array_equal(got[-1], frames[-1]) and w6[0][2] > 0


# ---- 8. the synchronous entries ---------------------------------------------------------------------------------------------------------
def _sync_batch(gpu, orc, fr):
    """clean | 2 header errors + damaged(within capacity) | header beyond repair | damaged(mixed) | clean -> (frames, expected frames,
    frame_rc, six counts per frame)"""
    hdr = gpu.header_encode(gpu.make_cfg(mode=1, **fr.kw), fr.n_raw)
    within = ("damaged", 35, tuple(ep.admissible(fr.ks[0])))
    mixed = ("damaged", 36)
    s_within, s_mixed, clean = stream_of(orc, fr, within), stream_of(orc, fr, mixed), stream_of(orc, fr, "clean")
    assert np.array_equal(clean[: len(hdr)], hdr)
    (e_within, w_within), (e_mixed, w_mixed) = expected_of(orc, fr, within), expected_of(orc, fr, mixed)
    assert w_within[1] == 0 and w_within[5] == w_within[4] > 0 and w_mixed[1] > 0 and 0 < w_mixed[5] < w_mixed[4]
    frames = [clean, _damage_header(s_within, 2), _damage_header(s_within, 9), s_mixed, clean]
    e1 = e_within.copy(); e1[: len(hdr)] = hdr                              # the header comes back as t3hip_header_encode's bytes
    want = [clean, e1, frames[2], e_mixed, clean]
    counts = [[0] * 6, [1] + w_within[1:], [0] * 6, [0] + w_mixed[1:], [0] * 6]
    return frames, want, [gpu.OK, gpu.OK, gpu.E_HEADER, gpu.E_RS, gpu.OK], counts


def test_synchronous_entries(gpu, orc):
    """The _dev and the host form, with and without T3_REPAIR_WRITE, at two strides: the frame whose header does not decode is untouched,
    reports E_HEADER and zero counts and splits the batch into two runs; a repairable header is rewritten; the host form leaves the
    stride gaps alone."""
    import torch
    fr = _frame("k20", "padded")
    frames, want, want_rc, want_counts = _sync_batch(gpu, orc, fr)
    nb, N = len(frames[0]), len(frames)
    for flags in (gpu.REPAIR_WRITE, 0):
        for stride in (nb + (nb & 1), round16(nb) + 32):
            data, spans = layout(frames, stride)
            buf = bounds.Buf(len(data), FILL, 0, data=data, name="batch", may_change=spans)
            rc, rcs, counts = gpu.repair_erasures_frames_dev(buf.ptr, nb // 9, stride, N, gpu.DecoderContext(mode=1).cfg_last_seen, flags,
                                                             torch.cuda.current_stream().cuda_stream)
            bounds.sync()
            assert rc == gpu.OK and rcs == want_rc and counts == want_counts, (flags, stride, rc, rcs, counts)
            got = buf.result()
            for f, (lo, hi) in enumerate(spans):
                bounds.check_equal(got[lo:hi], want[f] if flags else frames[f], FILL, "repair_erasures_frames_dev frame %d flags %d" % (f, flags))
            w, _ = layout(frames, stride)
            w = np.concatenate([w, np.full(stride - nb, GAP, np.uint8)]).reshape(N, stride)
            ctx = gpu.DecoderContext(mode=1)
            rc, rcs, counts = gpu.repair_erasures_frames(w, ctx, flags)
            assert rc == gpu.OK and rcs == want_rc and counts == want_counts, (flags, stride, "host", rc, rcs, counts)
            assert ctx.cfg_last_seen.profile == rp.CONFIGS["k20"]["profile"]
            for f in range(N):
                assert np.array_equal(w[f, :nb], want[f] if flags else frames[f]) and (w[f, nb:] == GAP).all(), (flags, stride, "host", f)
    flat, _ = layout(frames, nb + (nb & 1))                                   # a flat array plus a stride: the last frame ends with its words
    rc, rcs, counts = gpu.repair_erasures_frames(flat, gpu.DecoderContext(mode=1), gpu.REPAIR_WRITE, stride=nb + (nb & 1))
    assert rc == gpu.OK and rcs == want_rc and counts == want_counts
    bad = np.stack([_damage_header(frames[0], 9)] * 2)                        # no header decodes: E_HEADER, nothing written
    rc, rcs, counts = gpu.repair_erasures_frames(bad, gpu.DecoderContext(mode=1))
    assert rc == gpu.E_HEADER and rcs == [gpu.E_HEADER] * 2 and counts == [[0] * 6] * 2 and np.array_equal(bad[0], _damage_header(frames[0], 9))
    with pytest.raises(gpu.T3Error) as e:                                     # seen->mode must be FIXED on entry
        gpu.repair_erasures_frames(flat, gpu.DecoderContext(mode=0), stride=nb + (nb & 1))
    assert e.value.code == gpu.E_ARG


# ---- 9. the C++ demo --------------------------------------------------------------------------------------------------------------------
def test_repair_erasures_frames_demo(gpu, orc, tmp_path):
    """tests/cpp/repair_erasures_frames_demo.cpp: a relay's loop over a file of N frames through repair_erasures_frames of
    include/ternary_codec_v6.hpp, built with g++ alone."""
    lib = os.path.join(ROOT, "ternary-image-codec_amd")
    exe = str(tmp_path / "repair_erasures_frames_demo")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "repair_erasures_frames_demo.cpp"),
                    "-L" + lib, "-lt3hip", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-o", exe], check=True)
    fr = _small_k20(gpu, orc, False)                                          # frames back to back in a file: an even byte count each
    frames, want, want_rc, want_counts = _sync_batch(gpu, orc, fr)
    fin, fout = str(tmp_path / "in.words"), str(tmp_path / "out.words")
    np.concatenate(frames).tofile(fin)
    out = json.loads(subprocess.run([exe, fin, str(len(frames)), fout], check=True, capture_output=True, text=True).stdout)
    assert out == {"ok": 0, "status": gpu.E_HEADER, "frames": [[rc] + c for rc, c in zip(want_rc, want_counts)]}, out
    assert np.array_equal(np.fromfile(fout, np.uint8), np.concatenate(want))
    np.concatenate(frames[:2]).tofile(fin)                                    # every frame clean afterwards
    out = json.loads(subprocess.run([exe, fin, "2", fout], check=True, capture_output=True, text=True).stdout)
    assert out == {"ok": 1, "status": 0, "frames": [[rc] + c for rc, c in zip(want_rc[:2], want_counts[:2])]}, out
    assert np.array_equal(np.fromfile(fout, np.uint8), np.concatenate(want[:2]))
    odd = _small_k20(gpu, orc, True)                                          # an odd frame byte size: refused, nothing done
    np.concatenate([stream_of(orc, odd, "clean")] * 2).tofile(fin)
    out = json.loads(subprocess.run([exe, fin, "2", fout], check=True, capture_output=True, text=True).stdout)
    assert out["ok"] == 0 and out["status"] == gpu.E_ARG, out
