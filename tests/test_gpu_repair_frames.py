"""GPU tests of the batched stream repair (include/t3hip.h, "repair of a batch of equal FIXED frames"): repair_frames_kernel<R> -- ONE
launch over the tile space of all frames -- for the framings the fused kernel serves, the loop of the single-frame body for the others,
and the synchronous entries.  The yardstick is expected(orc, fr, received) of tests/test_repair_semantics.py, proven there on the CPU;
what a batch does to frame f -- bytes and the four words -- is what t3hip_repair_frame_async does to that frame alone.  One guarded
buffer per batch (tests/bounds.py): the frames' bytes may change, the gaps of a stride and the guards may not.  Byte work: every
comparison is exact."""
import json
import os
import subprocess

import numpy as np
import pytest

import bounds
import rs_patterns as rp
from test_gpu_repair import _damage_header, _frame, run as run_single
from test_repair_semantics import FUSED, SWEEP, expected

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = bounds.FILLS[0]
GAP = 0x3C                                                                # what the bytes of a stride behind a frame hold
_STREAMS, _EXPECTED = {}, {}


def stream_of(fr, case):
    """(received stream flat, M) of a frame's case, built once; 'clean' is the frame itself"""
    key = (fr.name, fr.n_px, case)
    if key not in _STREAMS:
        s, M = (fr.clean, 0) if case == "clean" else fr.stream(case)[:2]
        _STREAMS[key] = (np.ascontiguousarray(s, np.uint8).reshape(-1).copy(), M)
    return _STREAMS[key]


def expected_of(orc, fr, case):
    """The yardstick's (R', [uncorrectable, blocks changed, bytes changed]) of a frame's case, computed once and never changed"""
    key = (fr.name, fr.n_px, case)
    if key not in _EXPECTED:
        e, w, _ = expected(orc, fr, stream_of(fr, case)[0])
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


def run_batch(gpu, fr, frames, flags, stride=None, offset=0, fill=FILL):
    """One t3hip_repair_frames_async over `frames` (flat byte arrays) in one guarded buffer -> ([each frame's bytes afterwards], [its
    four words]); guards and gaps are checked, every byte of a frame may change."""
    import torch
    cfg = gpu.make_cfg(mode=1, **fr.kw)
    nb, N = len(frames[0]), len(frames)
    p = gpu.repair_frames_plan(fr.n_raw, N, cfg)
    assert p.in_bytes == nb and p.stride_min == nb + (nb & 1)
    stride = p.stride_min if stride is None else stride
    data, spans = layout(frames, stride)
    buf = bounds.Buf(len(data), fill, offset, data=data, name="batch", may_change=spans)
    ver = torch.full((4 * N,), 7, dtype=torch.int32, device="cuda")
    gpu.repair_frames_async(buf.ptr, nb // 9, stride, N, cfg, fr.n_raw, flags, ver.data_ptr(), torch.cuda.current_stream().cuda_stream)
    bounds.sync()
    got = buf.result()
    return [got[lo:hi] for lo, hi in spans], ver.cpu().numpy().reshape(N, 4).tolist()


def check_batch(gpu, orc, fr, cases, tag, **kw):
    """A batch of a frame's cases under T3_REPAIR_WRITE against the yardstick -> (bytes, words) per frame"""
    got, ver = run_batch(gpu, fr, [stream_of(fr, c)[0] for c in cases], gpu.REPAIR_WRITE, **kw)
    for f, c in enumerate(cases):
        exp, words = expected_of(orc, fr, c)
        assert ver[f] == [0] + words, (tag, f, c, "words", ver[f], words)
        bounds.check_equal(got[f], exp, kw.get("fill", FILL), "repaired %s frame %d (%s)" % (tag, f, c))
    return got, ver


# ---- the main sweep ---------------------------------------------------------------------------------------------------------------------
SWEEP_CASES = [(n, w) for w in ("small", "padded") for n in SWEEP] + [("k20", "full"), ("2d_64x64_k20", "full")]


@pytest.mark.parametrize("name,what", SWEEP_CASES)
def test_batch_sweep(gpu, orc, name, what):
    """Every framing: the CASES of the size, a clean frame and the first case again, at the smallest stride and at a 16-byte one with
    gaps; bytes and words are the yardstick's and those of the single-frame entry on each frame alone."""
    fr = _frame(name, what)
    cases = list(rp.CASES[what]) + ["clean", rp.CASES[what][0]]
    p = gpu.repair_frames_plan(fr.n_raw, len(cases), gpu.make_cfg(mode=1, **fr.kw))
    assert p.one_launch == (1 if name in FUSED else 0) and p.path == p.one_launch
    alone = {c: run_single(gpu, fr, stream_of(fr, c)[0], gpu.REPAIR_WRITE) for c in set(cases)}
    for stride in (p.stride_min, round16(p.in_bytes) + 32):
        got, ver = check_batch(gpu, orc, fr, cases, (name, what, stride), stride=stride)
        for f, c in enumerate(cases):
            assert ver[f] == alone[c][1] and np.array_equal(got[f], alone[c][0]), (name, what, stride, f, c, "single-frame entry")
    assert expected_of(orc, fr, "clean")[1] == [0, 0, 0] and expected_of(orc, fr, cases[0])[1][0] == stream_of(fr, cases[0])[1]


@pytest.mark.parametrize("name", ("k20", "k20_beacon83"))
def test_dry_run_and_second_repair(gpu, orc, name):
    """Without T3_REPAIR_WRITE: the same words, the buffer unchanged.  A repair of the repaired batch: [0, M_f, 0, 0], nothing written."""
    fr = _frame(name, "padded")
    cases = list(rp.CASES["padded"]) + ["clean", rp.CASES["padded"][0]]
    frames = [stream_of(fr, c)[0] for c in cases]
    got, ver = run_batch(gpu, fr, frames, 0)
    for f, c in enumerate(cases):
        assert ver[f] == [0] + expected_of(orc, fr, c)[1], (name, f, c, "dry run", ver[f])
        assert np.array_equal(got[f], frames[f]), (name, f, c, "dry run wrote")
    repaired = [expected_of(orc, fr, c)[0] for c in cases]
    got, ver = run_batch(gpu, fr, repaired, gpu.REPAIR_WRITE)
    for f, c in enumerate(cases):
        assert ver[f] == [0, expected_of(orc, fr, c)[1][0], 0, 0], (name, f, c, "second repair", ver[f])
        assert np.array_equal(got[f], repaired[f]), (name, f, c, "second repair wrote")


def test_isolation(gpu, orc):
    """clean, far1000, clean: the damaged frame changes neither its neighbours' words nor their bytes."""
    fr = _frame("k20", "full")
    got, ver = check_batch(gpu, orc, fr, ["clean", "far1000", "clean"], "isolation")
    clean = stream_of(fr, "clean")[0]
    assert ver[0] == ver[2] == [0, 0, 0, 0] and np.array_equal(got[0], clean) and np.array_equal(got[2], clean)
    assert ver[1][1] == 1000 and ver[1][2] > 0


def test_header_word(gpu, orc):
    """One symbol of frame 1's header changed: its word 0 is 1, every other frame's 0; all bodies are repaired, no header is touched."""
    fr = _frame("k20", "padded")
    cases = ["sched", "sched", "far2", "clean"]
    frames = [stream_of(fr, c)[0].copy() for c in cases]
    frames[1][5] = (frames[1][5] + 1) % 27
    got, ver = run_batch(gpu, fr, frames, gpu.REPAIR_WRITE)
    for f, c in enumerate(cases):
        exp, words = expected_of(orc, fr, c)
        want = exp.copy(); want[: int(fr.L.header_syms)] = frames[f][: int(fr.L.header_syms)]
        assert ver[f] == [1 if f == 1 else 0] + words, (f, c, ver[f])
        bounds.check_equal(got[f], want, FILL, "header word, frame %d" % f)


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
    assert p.in_bytes % 2 == 1 and p.stride_min == p.in_bytes + 1 and p.one_launch == 1
    for fill in bounds.FILLS:
        check_batch(gpu, orc, fr, ["sched", "far1", "clean", "far2"], ("addresses", fill), offset=2, fill=fill)


def test_frame_crossing(gpu, orc):
    """Frames of 7 tiles, the last ragged and the pixel count odd, so many of them that every workgroup walks more than two tiles and
    changes frame at points that do not line up with the grid; four streams cycled over the frames.  Every frame's bytes and words are
    the yardstick's: the per-frame sums of words 1 to 3 are exact, so a missed or doubled flush at a frame change shows."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n_frames = -(-(9 * cus + 1) // 7)
    cfg = gpu.make_cfg(mode=1, **rp.CONFIGS["k20"])
    fr = rp.Frame(orc, lambda n_raw: gpu.plan(n_raw, cfg), "k20", 7 * 2160 - 1001, 104)
    p = gpu.repair_frames_plan(fr.n_raw, n_frames, cfg)
    assert p.one_launch == 1 and p.tiles_per_frame == 7 and n_frames * 7 >= 3 * 3 * cus
    cycle = ("sched", "far1", "far2", "clean")
    cases = [cycle[f % 4] for f in range(n_frames)]
    got, ver = check_batch(gpu, orc, fr, cases, "crossing")
    assert expected_of(orc, fr, "sched")[1][1] > 0 and expected_of(orc, fr, "far2")[1][0] == 2


# ---- the synchronous entries ------------------------------------------------------------------------------------------------------------
def _sync_batch(gpu, orc, fr):
    """clean | 2 header errors + sched | header beyond repair | far2 | clean -> (frames, expected frames, frame_rc, counts)"""
    hdr = gpu.header_encode(gpu.make_cfg(mode=1, **fr.kw), fr.n_raw)
    sched, far2, clean = stream_of(fr, "sched")[0], stream_of(fr, "far2")[0], stream_of(fr, "clean")[0]
    assert np.array_equal(clean[: len(hdr)], hdr)
    frames = [clean, _damage_header(sched, 2), _damage_header(sched, 9), far2, clean]
    e1 = expected_of(orc, fr, "sched")[0].copy(); e1[: len(hdr)] = hdr       # the header comes back as t3hip_header_encode's bytes
    want = [clean, e1, frames[2], expected_of(orc, fr, "far2")[0], clean]
    counts = [[0, 0, 0, 0], [1] + expected_of(orc, fr, "sched")[1], [0, 0, 0, 0], [0] + expected_of(orc, fr, "far2")[1], [0, 0, 0, 0]]
    return frames, want, [gpu.OK, gpu.OK, gpu.E_HEADER, gpu.E_RS, gpu.OK], counts


def test_synchronous_entries(gpu, orc):
    """The _dev and the host form, with and without T3_REPAIR_WRITE: the frame whose header does not decode is untouched, reports
    E_HEADER and zero counts and splits the batch into two runs; a repairable header is rewritten."""
    import torch
    fr = _frame("k20", "padded")
    frames, want, want_rc, want_counts = _sync_batch(gpu, orc, fr)
    nb, N = len(frames[0]), len(frames)
    for flags in (gpu.REPAIR_WRITE, 0):
        for stride in (nb + (nb & 1), round16(nb) + 32):
            data, spans = layout(frames, stride)
            buf = bounds.Buf(len(data), FILL, 0, data=data, name="batch", may_change=spans)
            rc, rcs, counts = gpu.repair_frames_dev(buf.ptr, nb // 9, stride, N, gpu.DecoderContext(mode=1).cfg_last_seen, flags, torch.cuda.current_stream().cuda_stream)
            bounds.sync()
            assert rc == gpu.OK and rcs == want_rc and counts == want_counts, (flags, stride, rc, rcs, counts)
            got = buf.result()
            for f, (lo, hi) in enumerate(spans):
                bounds.check_equal(got[lo:hi], want[f] if flags else frames[f], FILL, "repair_frames_dev frame %d flags %d" % (f, flags))
            w, _ = layout(frames, stride)
            w = np.concatenate([w, np.full(stride - nb, GAP, np.uint8)]).reshape(N, stride)
            ctx = gpu.DecoderContext(mode=1)
            rc, rcs, counts = gpu.repair_frames(w, ctx, flags)
            assert rc == gpu.OK and rcs == want_rc and counts == want_counts, (flags, stride, "host", rc, rcs, counts)
            assert ctx.cfg_last_seen.profile == rp.CONFIGS["k20"]["profile"]
            for f in range(N):
                assert np.array_equal(w[f, :nb], want[f] if flags else frames[f]) and (w[f, nb:] == GAP).all(), (flags, stride, "host", f)
    flat, _ = layout(frames, nb + (nb & 1))                                   # a flat array plus a stride: the last frame ends with its words
    rc, rcs, counts = gpu.repair_frames(flat, gpu.DecoderContext(mode=1), gpu.REPAIR_WRITE, stride=nb + (nb & 1))
    assert rc == gpu.OK and rcs == want_rc and counts == want_counts
    bad = np.stack([_damage_header(frames[0], 9)] * 2)                        # no header decodes: E_HEADER, nothing written
    rc, rcs, counts = gpu.repair_frames(bad, gpu.DecoderContext(mode=1))
    assert rc == gpu.E_HEADER and rcs == [gpu.E_HEADER] * 2 and counts == [[0, 0, 0, 0]] * 2 and np.array_equal(bad[0], _damage_header(frames[0], 9))
    with pytest.raises(gpu.T3Error) as e:                                     # seen->mode must be FIXED on entry
        gpu.repair_frames(flat, gpu.DecoderContext(mode=0), stride=nb + (nb & 1))
    assert e.value.code == gpu.E_ARG


def test_repair_frames_demo(gpu, orc, tmp_path):
    """tests/cpp/repair_frames_demo.cpp: a relay's loop over a file of N frames through repair_frames of include/ternary_codec_v6.hpp,
    built with g++ alone."""
    lib = os.path.join(ROOT, "ternary-image-codec_amd")
    exe = str(tmp_path / "repair_frames_demo")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "repair_frames_demo.cpp"),
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
    np.concatenate([stream_of(odd, "clean")[0]] * 2).tofile(fin)
    out = json.loads(subprocess.run([exe, fin, "2", fout], check=True, capture_output=True, text=True).stdout)
    assert out["ok"] == 0 and out["status"] == gpu.E_ARG, out


# ---- two configurations in one batch ----------------------------------------------------------------------------------------------------
SCR_A, SCR_B = (1, 1, 1), (2, 5, 1)                                       # the scrambler seeds of configurations A and B


def next_table(hdr):
    """the scrambler's next-state table as a FIXED header carries it: ext[26], the last data symbol of its third block"""
    e = int(hdr[69])
    return [e % 3, e // 3 % 3, e // 9 % 3]


def two_configurations(gpu, orc, n_px):
    """The k20 frame of n_px pixels under the seeds of A and of B -> (frame A, frame B); asserts that the profile, n_raw and layout are
    one and that the two next-state tables differ"""
    frs = []
    for scr in (SCR_A, SCR_B):
        cfg = gpu.make_cfg(mode=1, **dict(rp.CONFIGS["k20"], seed=scr))
        frs.append(rp.Frame(orc, lambda n_raw, cfg=cfg: gpu.plan(n_raw, cfg), "k20", n_px, 105, scr=scr))
    A, B = frs
    ha, hb = (gpu.header_encode(gpu.make_cfg(mode=1, **fr.kw), fr.n_raw) for fr in frs)
    assert A.n_raw == B.n_raw and len(A.clean.reshape(-1)) == len(B.clean.reshape(-1)) and next_table(ha) != next_table(hb), (next_table(ha), next_table(hb))
    p = gpu.repair_frames_plan(A.n_raw, 2, gpu.make_cfg(mode=1, **A.kw))
    assert p.one_launch == 1 and p.path == 1 and p.tiles_per_frame >= 2
    return A, B


def test_two_configurations_in_one_batch(gpu, orc):
    """A A B B A: five frames of one profile and one n_raw_words whose scrambler seeds differ, through the _dev and the host entry, plain
    and with erasures, with and without T3_REPAIR_WRITE.  The runs are 2, 2, 1 -- the one launch twice and the single-frame body inside a
    batch -- and every frame's bytes, counts and code are the yardstick's for that frame alone."""
    import torch
    import erasure_patterns as ep
    from test_gpu_erasure_frames import _kinds
    A, B = two_configurations(gpu, orc, _small_k20(gpu, orc, False).n_px)
    order = (A, A, B, B, A)
    for era in (False, True):
        if era:
            received = [ep.damage_frame(orc, fr, seed, only=_kinds(fr, seed))[0] for fr, seed in zip(order, (81, 82, 83, 84, 81))]
            received[1] = A.clean
            yard = [ep.expected_erasures(orc, fr, s)[:2] for fr, s in zip(order, received)]
            want_counts = [[0] + w[1:] for _, w in yard]
            assert any((np.asarray(s) > 26).any() for s in received) and want_counts[2] != want_counts[0]
        else:
            received = [fr.stream(c)[0] for fr, c in zip(order, ("sched", "far2", "sched", "far1", "sched"))]
            received[4] = A.clean
            yard = [expected(orc, fr, s)[:2] for fr, s in zip(order, received)]
            want_counts = [[0] + w for _, w in yard]
        frames = [np.ascontiguousarray(s, np.uint8).reshape(-1) for s in received]
        want = [np.asarray(e).reshape(-1) for e, _ in yard]
        want_rc = [gpu.E_RS if c[1] else gpu.OK for c in want_counts]
        assert gpu.E_RS in want_rc and gpu.OK in want_rc and any(c[3] for c in want_counts)
        nb, N = len(frames[0]), len(frames)
        stride = nb + (nb & 1)
        dev = gpu.repair_erasures_frames_dev if era else gpu.repair_frames_dev
        host = gpu.repair_erasures_frames if era else gpu.repair_frames
        for flags in (gpu.REPAIR_WRITE, 0):
            data, spans = layout(frames, stride)
            buf = bounds.Buf(len(data), FILL, 0, data=data, name="batch", may_change=spans)
            seen = gpu.DecoderContext(mode=1).cfg_last_seen
            rc, rcs, counts = dev(buf.ptr, nb // 9, stride, N, seen, flags, torch.cuda.current_stream().cuda_stream)
            bounds.sync()
            assert rc == gpu.OK and rcs == want_rc and counts == want_counts, (era, flags, rc, rcs, counts, want_counts)
            got = buf.result()
            for f, (lo, hi) in enumerate(spans):
                bounds.check_equal(got[lo:hi], want[f] if flags else frames[f], FILL, "two configurations, era %d flags %d frame %d" % (era, flags, f))
            w, _ = layout(frames, stride)
            w = np.concatenate([w, np.full(stride - nb, GAP, np.uint8)]).reshape(N, stride)
            rc, rcs, counts = host(w, gpu.DecoderContext(mode=1), flags)
            assert rc == gpu.OK and rcs == want_rc and counts == want_counts, (era, flags, "host", rc, rcs, counts)
            for f in range(N):
                assert np.array_equal(w[f, :nb], want[f] if flags else frames[f]) and (w[f, nb:] == GAP).all(), (era, flags, "host", f)
