"""The records and payload CRCs of N equal frames in one pass (t3hip_frame_records_dev, t3hip_crc32_frames[_dev]) against the
single-frame entry, zlib and the oracle's symbol sum.

Every frame is a stretch of ONE random buffer of symbols 0..26: frame f is the n_bytes at f * stride of it, so the gaps between the
frames and the bytes behind the last one are random too -- a kernel that read a neighbour's bytes, or past its frame's end, would change
a result.  The records and the scratch sit in guarded buffers (tests/bounds.py)."""
import importlib
import json
import os
import subprocess
import zlib

import numpy as np
import pytest

import bounds

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAP = 4112                                   # the second stride: r16(bytes) + this
KNOBS = ("T3HIP_CRC_ATOMICS", "T3HIP_CRC_TABLES", "T3HIP_CRC_BLOCKED")


def r16(x):
    return (x + 15) & ~15


def words_for(rounds, tail):
    """A word count n near `rounds` rounds with 9 n = 2048 m + tail (tests/test_crc_tail.py)."""
    base = 2048 * rounds // 9
    n = base + ((tail * pow(9, -1, 2048) - base) % 2048)
    assert (9 * n) % 2048 == tail
    return n


def video_words(t3):
    """Coded words of a FIXED RS(26,20) 854 x 480 frame: the batch workload."""
    return t3.encoded_words((854 * 480 + 1) // 2, t3.make_cfg(profile=2, uep=2, mode=t3.MODE_FIXED))


# (rounds, rest): the smallest shapes at which each branch can go wrong
SMALL = {"tables": (40, 7), "fp4_min": (64, 0), "fp4_min_rest": (64, 2047), "edge_lo": (255, 3), "edge_hi": (256, 16), "video": None,
         "five_words": 5, "no_words": 0}
LARGE = {"level1": (16383, 1), "level0": (16384, 54)}
CASES = [(k, n) for k in SMALL for n in (1, 2, 3, 17)] + [(k, 2) for k in LARGE]


def n_words_of(t3, key):
    v = {**SMALL, **LARGE}[key]
    return video_words(t3) if v is None else words_for(*v) if isinstance(v, tuple) else v


@pytest.fixture(scope="module")
def stream(gpu):
    """The one random buffer, host and device: room for the largest batch at the wider stride (under 75 MB)."""
    import torch
    need = max(n * (r16(9 * n_words_of(gpu, k)) + GAP) for k, n in CASES) + 4096
    assert need < 75e6
    host = np.random.default_rng(23).integers(0, 27, size=need, dtype=np.uint8)
    return host, torch.from_numpy(host).cuda()


_single = {}


def single_records(gpu, dev, n_words, stride, n, first, step):
    """What the parent's entry writes: frame_record_dev for every frame alone, with its index (computed once per shape)."""
    import torch
    key = (n_words, stride, n, first, step)
    if key not in _single:
        cfg = gpu.make_cfg(profile=2, uep=2, mode=gpu.MODE_FIXED)
        recs = torch.zeros((n, gpu.FRAME_RECORD_BYTES), dtype=torch.uint8, device="cuda")
        scr = torch.zeros(gpu.frame_record_scratch_bytes(n_words), dtype=torch.uint8, device="cuda")
        for f in range(n):
            gpu.frame_record_dev(dev.data_ptr() + f * stride, n_words, first + f * step, cfg, recs[f].data_ptr(), scr.data_ptr(), scr.numel())
        torch.cuda.synchronize()
        _single[key] = recs.cpu().numpy().reshape(-1)
    return _single[key]


_host_sums = {}


def host_sums(orc, host, n_words, stride, n):
    """zlib's CRC-32 and the oracle's symbol sum of every frame (computed once per shape)."""
    key = (n_words, stride, n)
    if key not in _host_sums:
        fr = [host[f * stride: f * stride + 9 * n_words] for f in range(n)]
        _host_sums[key] = [(zlib.crc32(p), orc.sym_sum(p) if len(p) else 0) for p in fr]
    return _host_sums[key]


def check_batch(gpu, orc, host, dev, n_words, n, stride, first, step, scratch_bytes, fill):
    cfg = gpu.make_cfg(profile=2, uep=2, mode=gpu.MODE_FIXED)
    recs = bounds.Buf(gpu.FRAME_RECORD_BYTES * n, fill, name="records")
    scr = bounds.Buf(scratch_bytes, fill, name="scratch")
    gpu.frame_records_dev(dev.data_ptr(), n_words, stride, n, first, step, cfg, recs.ptr, scr.ptr, scratch_bytes)
    got, _ = bounds.results(recs, scr)                                        # one synchronise; guards of both checked
    bounds.check_equal(got, single_records(gpu, dev, n_words, stride, n, first, step), fill, "records vs frame_record_dev")
    sums = host_sums(orc, host, n_words, stride, n)
    for f in range(n):
        r = gpu.FrameRecord.from_buffer_copy(got[f * 96:(f + 1) * 96].tobytes())
        payload = host[f * stride: f * stride + 9 * n_words]
        assert (r.frame_idx, r.n_words, r.byte_offset) == (first + f * step, n_words, 0), (f, n_words)
        assert (r.crc32, r.sym_sum) == sums[f], (f, n_words, stride, scratch_bytes)
        assert (r.profile, r.mode) == (2, gpu.MODE_FIXED)
        k = min(54, len(payload))
        assert list(r.header_syms)[:k] == list(payload[:k]) and not any(list(r.header_syms)[k:])


@pytest.mark.parametrize("key,n", CASES)
def test_records(gpu, orc, stream, key, n):
    """Both strides, the full scratch and 16 bytes per frame (accumulators), index steps 1 and 8, both fills."""
    host, dev = stream
    n_words = n_words_of(gpu, key)
    tight = r16(9 * n_words)
    for stride, first, step in ((tight, 3, 1), (tight + GAP, 5, 8)):
        for i, scratch_bytes in enumerate((gpu.frame_records_scratch_bytes(n_words, n), 16 * n)):
            for fill in (bounds.FILLS if key in SMALL else bounds.FILLS[i: i + 1]):
                check_batch(gpu, orc, host, dev, n_words, n, stride, first, step, scratch_bytes, fill)


def test_sizes_reach_the_levels(gpu):
    """The sizes above reach the lowest stride level, level 0 and at least one between, on this part (W is read from the plan)."""
    import torch
    slots = 8 * torch.cuda.get_device_properties(0).multi_processor_count
    w_of = lambda l: max(4, (slots >> l) & ~3)
    seen = set()
    for key in list(SMALL) + list(LARGE):
        p = gpu.frame_records_plan(n_words_of(gpu, key), 2)                   # n_cu = 0: this device
        if p.form == gpu.RECORDS_FP4:
            seen.add(p.stride_waves)
            assert p.one_pass == 1 and p.partials_per_frame == p.wgs_per_frame > 0
    assert len(seen) >= 3 and w_of(7) in seen and w_of(0) in seen, (sorted(seen), slots)
    assert gpu.frame_records_plan(n_words_of(gpu, "tables"), 2).form == gpu.RECORDS_TABLES


def test_no_frames_touches_nothing(gpu, stream):
    host, dev = stream
    cfg = gpu.make_cfg(profile=2, uep=2, mode=gpu.MODE_FIXED)
    recs = bounds.Buf(96, 0xA5, name="records"); scr = bounds.Buf(64, 0xA5, name="scratch")
    gpu.frame_records_dev(dev.data_ptr(), 4861, r16(9 * 4861), 0, 0, 1, cfg, recs.ptr, scr.ptr, 64)
    bounds.sync()
    recs.untouched(); scr.untouched()


@pytest.mark.parametrize("knob", KNOBS)
def test_records_knobs(gpu, orc, stream, knob, monkeypatch):
    """The measurement knobs give the same records: accumulators although there is room for partials, the table kernel for every
    frame, the loop of the single-frame entry."""
    host, dev = stream
    n_words = n_words_of(gpu, "edge_lo")
    single_records(gpu, dev, n_words, r16(9 * n_words), 3, 3, 1)              # what check_batch compares with: written without the knob
    monkeypatch.setenv(knob, "1")
    p = gpu.frame_records_plan(n_words, 3)
    assert (p.one_pass, p.form, p.partials_per_frame) == {"T3HIP_CRC_ATOMICS": (1, 1, 0), "T3HIP_CRC_TABLES": (1, 0, 0), "T3HIP_CRC_BLOCKED": (0, 1, p.wgs_per_frame)}[knob]
    for scratch_bytes in (gpu.frame_records_scratch_bytes(n_words, 3), 48):
        check_batch(gpu, orc, host, dev, n_words, 3, r16(9 * n_words), 3, 1, scratch_bytes, 0xA5)
    assert gpu.crc32_frames_dev(dev.data_ptr(), 9 * n_words, r16(9 * n_words), 3) == [c for c, _ in host_sums(orc, host, n_words, r16(9 * n_words), 3)]


@pytest.mark.parametrize("key", list(SMALL) + list(LARGE))
def test_crc32_frames(gpu, stream, key):
    """The containers' payload CRC of N equal buffers against zlib: device buffers at both strides, host arrays at unrelated addresses,
    n_frames 0 and 1 too, and a length that is no multiple of 9."""
    host, dev = stream
    n_words = n_words_of(gpu, key)
    for n_bytes in (9 * n_words, 9 * n_words + 5):
        for n in ((0, 1, 2) if key in LARGE else (0, 1, 3, 17)):
            for stride in (r16(n_bytes), r16(n_bytes) + GAP):
                want = [zlib.crc32(host[f * stride: f * stride + n_bytes]) if n_bytes else 0 for f in range(n)]
                assert gpu.crc32_frames_dev(dev.data_ptr(), n_bytes, stride, n) == want, (n_bytes, n, stride)
            if n <= 3:
                arrays = [host[f * stride: f * stride + n_bytes].copy() for f in range(n)]        # stride: the wider one
                assert gpu.crc32_frames(arrays) == want, (n_bytes, n)


def test_local_records(gpu, stream):
    """superframe.local_records for rank 1 of 4: its frames are 1, 5, 9; assembled with the other ranks' records into the index."""
    import torch
    host, dev = stream
    sf = importlib.import_module(gpu.__name__ + ".superframe")
    n_words, n_local, world = n_words_of(gpu, "edge_hi"), 3, 4
    stride = r16(9 * n_words)
    cfg = gpu.make_cfg(profile=2, uep=2, mode=gpu.MODE_FIXED)
    scr = torch.empty(gpu.frame_records_scratch_bytes(n_words, n_local), dtype=torch.uint8, device="cuda")
    gathered = torch.zeros((world, n_local, gpu.FRAME_RECORD_BYTES), dtype=torch.uint8, device="cuda")
    for rank in range(world):                                                 # (one process plays every rank; the gather is rank-major)
        assert sf.frames_of_rank(world * n_local, rank, world) == [rank + i * world for i in range(n_local)]
        sf.local_records(dev.data_ptr(), n_words, stride, n_local, rank, world, cfg, gathered[rank].data_ptr(), scr.data_ptr(), scr.numel())
    torch.cuda.synchronize()
    index = sf.assemble_index(gathered.reshape(-1, gpu.FRAME_RECORD_BYTES), 100)
    assert [r.frame_idx for r in index] == list(range(world * n_local))
    assert [r.byte_offset for r in index] == [100 + 9 * n_words * i for i in range(world * n_local)]
    for r in index:                                                           # frame idx = rank + i * world was local frame i of every rank
        i = r.frame_idx // world
        assert r.crc32 == zlib.crc32(host[i * stride: i * stride + 9 * n_words]) and r.n_words == n_words


def test_t3v_bytes_takes_the_batch_crc(gpu, monkeypatch):
    """containers.t3v_bytes: seven equal frames (one crc32_frames call) give the bytes that zlib's CRCs give; a list of mixed sizes
    still goes frame by frame and matches too."""
    cont = importlib.import_module(gpu.__name__ + ".containers")
    rng = np.random.default_rng(5)
    equal = [rng.integers(0, 27, size=9 * 20000, dtype=np.uint8) for _ in range(7)]
    mixed = equal[:2] + [equal[2][: 9 * 777], np.zeros(0, np.uint8)] + equal[3:5]
    calls = []
    batch, single = cont._device_crc32_frames, cont._device_crc32
    monkeypatch.setattr(cont, "_device_crc32_frames", lambda fr: calls.append(("frames", len(fr))) or batch(fr))
    monkeypatch.setattr(cont, "_device_crc32", lambda b: calls.append(("one", b.size)) or single(b))
    for frames, metas in ((equal, ()), (equal, [b"m%d" % i for i in range(7)]), (mixed, ())):
        del calls[:]
        crcs = [zlib.crc32(f.tobytes()) for f in frames]
        want = cont.t3v_bytes(27, 854, 480, frames, b'{"g":1}', metas, payload_crcs=crcs)
        assert not calls
        assert cont.t3v_bytes(27, 854, 480, frames, b'{"g":1}', metas) == want
        assert calls == ([("frames", 7)] if frames is equal else [("one", f.size) for f in frames if f.size])


def test_frame_records_demo(gpu, orc, tmp_path):
    """tests/cpp/frame_records_demo.cpp: encode_frames -> t3hip_frame_records_dev -> t3hip_index_assemble -> t3v_write_crc with the
    records' CRCs -> t3v_read_frame, through the C++ headers."""
    import oracle_lib as ol
    lib = os.path.join(ROOT, "ternary-image-codec_amd"); exe = os.path.join(str(tmp_path), "frame_records_demo")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include", "compat"),
                    "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "frame_records_demo.cpp"), "-L" + lib, "-lt3hip",
                    "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-o", exe], check=True)
    n, n_px = 5, 4861
    px = [orc.lcg_pixels(n_px, seed=100 + f) for f in range(n)]
    cfg = ol.make_cfg(profile=2, uep=2, mode=1)
    want = []
    for f in range(n):
        rc, w = orc.encode_frame(px[f], cfg); assert rc == 0
        want.append(np.ascontiguousarray(w, np.uint8).reshape(-1))
    p = lambda name: os.path.join(str(tmp_path), name)
    np.concatenate(px).tofile(p("in.px"))
    r = subprocess.run([exe, str(n), str(n_px), p("in.px"), p("out.t3v"), p("recs")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    info = json.loads(r.stdout.strip().splitlines()[-1])
    words = len(want[0]) // 9
    assert info == {"frames": n, "words": words, "read_ok": n}
    recs = gpu.index_assemble(np.fromfile(p("recs"), np.uint8), 0)
    off = 26 + 20 * n
    for f, rec in enumerate(recs):
        assert (rec.frame_idx, rec.n_words, rec.crc32, rec.sym_sum) == (f, words, zlib.crc32(want[f]), orc.sym_sum(want[f]))
    cont = importlib.import_module(gpu.__name__ + ".containers")
    assert open(p("out.t3v"), "rb").read() == cont.t3v_bytes(27, 854, 480, want, b"", (), payload_crcs=[zlib.crc32(w) for w in want])
    assert [rec.byte_offset for rec in gpu.index_assemble(np.fromfile(p("recs"), np.uint8), off)] == [off + 9 * words * f for f in range(n)]
