"""Batches of equal frames on the device (include/t3hip.h, "batches of equal frames"): N frames of one configuration and size encoded
or decoded by one call -- one kernel launch where the fused single-k kernels serve the framing, a loop of the single-frame entries
elsewhere.  The yardstick is the CPU oracle, frame by frame (encode_frame, decode_frame, rgb_to_quant / quant_to_rgb); one more
assertion per test holds the batch against a loop of single-frame GPU calls.  Every buffer carries 0xA5 in the gaps of its strides and
in a guard in front of and behind the batch, and the tests look at every one of those bytes."""
import functools
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as ol

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD, FILL = 4096, 0xA5
K20 = dict(profile=2, uep=2)
# (frames, pixels): two tiles and a ragged one with a pad pixel; exactly one decoder tile; less than a tile; more frames than resident
# workgroups (frame ends and header checks by many workgroups); two 854 x 480 frames
SHAPES = [(3, 4861), (4, 2160), (5, 100), (1000, 334), (2, 854 * 480)]
PER_FRAME = {"p5_tile64_luma": dict(profile=4, uep="luma", tile=(64, 64)), "p2_beacon83": dict(profile=1, uep=1, beacon=(83, 2, 1))}


def r16(x):
    return (x + 15) & ~15


def frame_pixels(n_frames, n_px, seed=0):
    """In-range pixel records, another stream per frame."""
    out = []
    for f in range(n_frames):
        rng = np.random.default_rng(1000 * seed + f + 1)
        px = np.zeros(n_px, ol.PIXEL_DT)
        px["Yq"] = rng.integers(0, 243, n_px); px["Cbq"] = rng.integers(-40, 41, n_px); px["Crq"] = rng.integers(-40, 41, n_px)
        out.append(px)
    return out


@functools.lru_cache(maxsize=None)
def oracle_batch(n_frames, n_px, mode, profile=2, seed=0):
    """(pixels per frame, oracle-coded words per frame as flat bytes): computed once, shared, never written to."""
    orc = ol.oracle()
    px = frame_pixels(n_frames, n_px, seed)
    cfg = ol.make_cfg(profile=profile, uep=profile, mode=mode)
    coded = []
    for p in px:
        rc, w = orc.encode_frame(p, cfg); assert rc == 0
        w = np.ascontiguousarray(w).reshape(-1).copy(); w.setflags(write=False)
        coded.append(w)
    for p in px:
        p.setflags(write=False)
    return px, coded


def to_dev(frames_bytes, stride):
    """The frames at `stride` behind a guard, everything else 0xA5 -> (device tensor, address of frame 0)."""
    import torch
    n = len(frames_bytes)
    buf = np.full(2 * GUARD + n * stride, FILL, np.uint8)
    for f, b in enumerate(frames_bytes):
        buf[GUARD + f * stride: GUARD + f * stride + len(b)] = b
    t = torch.from_numpy(buf).cuda()
    return t, t.data_ptr() + GUARD


def dev_out(n, stride):
    import torch
    t = torch.full((2 * GUARD + n * stride,), FILL, dtype=torch.uint8, device="cuda")
    return t, t.data_ptr() + GUARD


def split_out(t, n, stride, used):
    """Host copy of an output batch: the frames' own bytes, after checking that every other byte -- the gap of every stride, the guards in
    front and behind -- still holds 0xA5."""
    b = t.cpu().numpy()
    mask = np.ones(len(b), bool)
    for f in range(n):
        mask[GUARD + f * stride: GUARD + f * stride + used] = False
    assert np.all(b[mask] == FILL), "a byte outside the frames' own bytes was written: %s" % np.flatnonzero(mask & (b != FILL))[:8]
    return [b[GUARD + f * stride: GUARD + f * stride + used] for f in range(n)]


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def encode_batch(gpu, units, n_units, fmt, cfg, extra):
    """units: per-frame input bytes.  Returns (plan, per-frame coded bytes), gaps and guards checked."""
    import torch
    n = len(units)
    p = gpu.frames_plan(False, n_units, n, cfg, fmt)
    ins, outs = p.in_stride_min + extra, p.out_stride_min + extra
    d_in, a_in = to_dev(units, ins)
    d_out, a_out = dev_out(n, outs)
    words = gpu.encode_frames_dev(a_in, n_units, fmt, ins, n, cfg, a_out, outs, stream())
    torch.cuda.synchronize()
    assert 9 * words == p.out_bytes
    return p, split_out(d_out, n, outs, p.out_bytes)


def encode_loop(gpu, units, n_units, fmt, cfg):
    """The same frames through the single-frame device entries, one call per frame."""
    import torch
    res = []
    cap = gpu.encoded_words(n_units if fmt == gpu.FRAMES_WORDS else (n_units + 1) // 2, cfg)
    for u in units:
        d = torch.from_numpy(np.ascontiguousarray(u)).cuda(); o = torch.zeros(9 * cap + 64, dtype=torch.uint8, device="cuda")
        fn = {gpu.FRAMES_WORDS: gpu.encode_profile_dev, gpu.FRAMES_PIXELS: gpu.encode_frame_dev, gpu.FRAMES_RGB: gpu.encode_rgb_dev}[fmt]
        w = fn(d.data_ptr(), n_units, cfg, o.data_ptr(), cap, stream())
        torch.cuda.synchronize()
        res.append(o[: 9 * w].cpu().numpy())
    return res


def decode_batch(gpu, coded, n_raw, fmt, cfg, extra, inject=None):
    """coded: per-frame stream bytes.  inject = (first_sym, n_blocks, t): 0..t symbol errors per block, per-frame seed, on the device.
    Returns (plan, the streams as decoded, per-frame output bytes, verdict words), gaps and guards checked."""
    import torch
    n = len(coded); n_in = len(coded[0]) // 9
    p = gpu.frames_plan(True, n_raw if fmt == gpu.FRAMES_WORDS else 2 * n_raw, n, cfg, fmt)
    ins, outs = r16(9 * n_in) + extra, p.out_stride_min + extra
    d_in, a_in = to_dev(coded, ins)
    if inject:
        for f in range(n):
            gpu.inject_errors_dev(a_in + f * ins, inject[0], inject[1], 77 + f, inject[2], stream())
    d_out, a_out = dev_out(n, outs)
    ver = torch.full((2 * n,), 7, dtype=torch.int32, device="cuda")
    gpu.decode_frames_async(a_in, n_in, ins, n, cfg, n_raw, a_out, outs, fmt, ver.data_ptr(), stream())
    torch.cuda.synchronize()
    seen = split_out(d_in, n, ins, 9 * n_in)                                         # (the input's gaps are not written either)
    return p, seen, split_out(d_out, n, outs, p.out_bytes), ver.cpu().numpy().tolist()


def decode_loop(gpu, coded, n_raw, fmt, cfg):
    import torch
    res, vers = [], []
    units = n_raw if fmt == gpu.FRAMES_WORDS else 2 * n_raw
    ub = {gpu.FRAMES_WORDS: 9, gpu.FRAMES_PIXELS: 6, gpu.FRAMES_RGB: 3}[fmt]
    for c in coded:
        d = torch.from_numpy(np.ascontiguousarray(c)).cuda(); o = torch.zeros(units * ub + 64, dtype=torch.uint8, device="cuda")
        ver = torch.full((2,), 7, dtype=torch.int32, device="cuda")
        if fmt == gpu.FRAMES_RGB: gpu.decode_rgb_async(d.data_ptr(), len(c) // 9, cfg, units, o.data_ptr(), ver.data_ptr(), stream())
        else: gpu.decode_frame_async(d.data_ptr(), len(c) // 9, cfg, n_raw, o.data_ptr(), units, ver.data_ptr(), fmt == gpu.FRAMES_PIXELS, stream())
        torch.cuda.synchronize()
        res.append(o[: units * ub].cpu().numpy()); vers += ver.cpu().numpy().tolist()
    return res, vers


# ---- encode ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [0, 4096 + 16])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("shape", SHAPES)
def test_encode_frames_pixels(gpu, orc, shape, mode, extra):
    """RS(26,20), COMPAT and FIXED, pixels in: every frame of the batch equals the oracle's encode of it, with minimal strides and with
    strides of minimum + 4096 + 16 whose gaps stay untouched."""
    n, n_px = shape
    px, want = oracle_batch(n, n_px, mode)
    cfg = gpu.make_cfg(mode=mode, **K20)
    p, got = encode_batch(gpu, [q.view(np.uint8) for q in px], n_px, gpu.FRAMES_PIXELS, cfg, extra)
    assert p.one_launch == 1
    for f in range(n):
        assert np.array_equal(got[f], want[f]), "frame %d differs from the oracle" % f
    loop = encode_loop(gpu, [q.view(np.uint8) for q in px], n_px, gpu.FRAMES_PIXELS, cfg)
    assert all(np.array_equal(a, b) for a, b in zip(got, loop)), "batch != loop of single-frame calls"


@pytest.mark.parametrize("profile", [0, 1, 3])
def test_encode_decode_frames_other_codes(gpu, orc, profile):
    """RS(26,24), (26,22), (26,18), FIXED, three frames of two full decoder tiles and 541 pixels: encode against the oracle; decode of
    streams with 0..t errors per block against the oracle's decode of the same streams."""
    k = {0: 24, 1: 22, 3: 18}[profile]
    n, n_px = 3, 108 * k * 2 + 541
    px, want = oracle_batch(n, n_px, 1, profile)
    cfg = gpu.make_cfg(profile=profile, uep=profile, mode=1)
    p, got = encode_batch(gpu, [q.view(np.uint8) for q in px], n_px, gpu.FRAMES_PIXELS, cfg, 0)
    assert p.one_launch == 1 and all(np.array_equal(a, b) for a, b in zip(got, want))
    assert all(np.array_equal(a, b) for a, b in zip(got, encode_loop(gpu, [q.view(np.uint8) for q in px], n_px, gpu.FRAMES_PIXELS, cfg)))
    n_raw = (n_px + 1) // 2; L = gpu.plan(n_raw, cfg)
    dp, seen, out, ver = decode_batch(gpu, want, n_raw, gpu.FRAMES_PIXELS, cfg, 4096 + 16, (L.header_syms, L.body_syms // 26, (26 - k) // 2))
    assert dp.one_launch == 1 and ver == [0] * (2 * n), ver
    for f in range(n):
        assert not np.array_equal(seen[f], want[f]), "no error was injected"
        rc, opx = orc.decode_frame(seen[f].reshape(-1, 9), ol.make_cfg(profile=profile, uep=profile, mode=1)); assert rc == 0
        assert np.array_equal(out[f], opx.view(np.uint8)), "frame %d differs from the oracle's decode" % f
    loop, lver = decode_loop(gpu, seen, n_raw, gpu.FRAMES_PIXELS, cfg)
    assert lver == ver and all(np.array_equal(a, b) for a, b in zip(out, loop))


@pytest.mark.parametrize("shape", [(3, 4861), (2, 854 * 480)])
def test_encode_frames_rgb(gpu, orc, shape):
    """RGB8 in: the io_image.hpp bridge fused into the batch launch, against the oracle's bridge + encode."""
    n, n_px = shape
    rgb = [orc.lcg_rgb(n_px, 40 + f) for f in range(n)]
    cfg = gpu.make_cfg(mode=1, **K20)
    p, got = encode_batch(gpu, rgb, n_px, gpu.FRAMES_RGB, cfg, 4096 + 16)
    assert p.one_launch == 1
    for f in range(n):
        rc, w = orc.encode_frame(orc.rgb_to_quant(rgb[f]), ol.make_cfg(mode=1, **K20)); assert rc == 0
        assert np.array_equal(got[f], np.ascontiguousarray(w).reshape(-1)), "frame %d differs from the oracle" % f
    assert all(np.array_equal(a, b) for a, b in zip(got, encode_loop(gpu, rgb, n_px, gpu.FRAMES_RGB, cfg))), "batch != loop of single-frame calls"


# ---- decode ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [0, 4096 + 16])
@pytest.mark.parametrize("shape", SHAPES)
def test_decode_frames(gpu, orc, shape, extra):
    """FIXED RS(26,20), streams with 0..3 symbol errors per block (inject_errors_dev, another seed per frame): pixel and RGB output equal
    the oracle's decode of the same streams (and its bridge), every verdict word 0, gaps and guards intact."""
    n, n_px = shape
    px, coded = oracle_batch(n, n_px, 1)
    cfg = gpu.make_cfg(mode=1, **K20); n_raw = (n_px + 1) // 2; L = gpu.plan(n_raw, cfg)
    inj = (L.header_syms, L.body_syms // 26, 3)
    p, seen, out, ver = decode_batch(gpu, coded, n_raw, gpu.FRAMES_PIXELS, cfg, extra, inj)
    assert p.one_launch == 1 and ver == [0] * (2 * n), [i for i, v in enumerate(ver) if v][:10]
    want = []
    for f in range(n):
        rc, opx = orc.decode_frame(seen[f].reshape(-1, 9), ol.make_cfg(mode=1, **K20)); assert rc == 0 and len(opx) == 2 * n_raw
        assert np.array_equal(opx[:n_px], px[f])
        want.append(opx)
        assert np.array_equal(out[f], opx.view(np.uint8)), "frame %d differs from the oracle's decode" % f
    assert sum(not np.array_equal(a, b) for a, b in zip(seen, coded)) >= min(n, 2), "no error was injected"
    pr, seen_r, out_r, ver_r = decode_batch(gpu, coded, n_raw, gpu.FRAMES_RGB, cfg, extra, inj)
    assert pr.one_launch == 1 and ver_r == [0] * (2 * n) and all(np.array_equal(a, b) for a, b in zip(seen, seen_r))
    for f in range(n):
        assert np.array_equal(out_r[f], orc.quant_to_rgb(want[f])), "RGB frame %d differs from the oracle's bridge" % f
    loop, lver = decode_loop(gpu, seen, n_raw, gpu.FRAMES_PIXELS, cfg)
    assert lver == ver and all(np.array_equal(a, b) for a, b in zip(out, loop)), "batch != loop of single-frame calls"
    loop_r, lver_r = decode_loop(gpu, seen, n_raw, gpu.FRAMES_RGB, cfg)
    assert lver_r == ver_r and all(np.array_equal(a, b) for a, b in zip(out_r, loop_r)), "RGB batch != loop of single-frame calls"


def test_one_damaged_frame(gpu, orc):
    """Frame j of five carries a block with more than t symbol errors, in a pattern the oracle rejects (t + 1 errors may land within t of
    another codeword: the pattern is tried on the CPU first): d_verdict[2 j + 1] >= 1, every other verdict word 0, every other frame's
    pixels the oracle's."""
    n, n_px, j = 5, 4861, 3
    px, coded = oracle_batch(n, n_px, 1)
    cfg = gpu.make_cfg(mode=1, **K20); n_raw = (n_px + 1) // 2; L = gpu.plan(n_raw, cfg)
    bad = None
    for add in range(1, 27):                                               # block 7 of band 2: its first five symbols moved by `add`
        cand = coded[j].copy(); o = L.header_syms + L.band_body_off[2] + 26 * 7
        cand[o: o + 5] = (cand[o: o + 5] + add) % 27
        rc, _ = orc.decode_frame(cand.reshape(-1, 9), ol.make_cfg(mode=1, **K20))
        if rc == gpu.E_RS:
            bad = cand; break
    assert bad is not None, "the oracle accepted every pattern"
    frames = [bad if f == j else coded[f] for f in range(n)]
    p, seen, out, ver = decode_batch(gpu, frames, n_raw, gpu.FRAMES_PIXELS, cfg, 4096 + 16)
    assert p.one_launch == 1
    assert ver[2 * j + 1] >= 1 and all(v == 0 for i, v in enumerate(ver) if i != 2 * j + 1), ver
    padded = np.zeros(2 * n_raw, ol.PIXEL_DT)
    for f in range(n):
        if f != j:
            padded[:n_px] = px[f]
            assert np.array_equal(out[f], padded.view(np.uint8)), "frame %d was touched by its neighbour's damage" % f
    loop, lver = decode_loop(gpu, frames, n_raw, gpu.FRAMES_PIXELS, cfg)
    assert [bool(v) for v in lver] == [bool(v) for v in ver] and all(np.array_equal(out[f], loop[f]) for f in range(n) if f != j)


def test_one_frame_with_another_header(gpu, orc):
    """Frame j was encoded with another scrambler seed: d_verdict[2 j] == 1, the other frames' header words 0 and their pixels right."""
    n, n_px, j = 5, 4861, 1
    px, coded = oracle_batch(n, n_px, 1)
    rc, other = orc.encode_frame(px[j], ol.make_cfg(mode=1, seed=(2, 1, 1), **K20)); assert rc == 0
    other = np.ascontiguousarray(other).reshape(-1)
    assert len(other) == len(coded[j])
    cfg = gpu.make_cfg(mode=1, **K20); n_raw = (n_px + 1) // 2
    frames = [other if f == j else coded[f] for f in range(n)]
    p, seen, out, ver = decode_batch(gpu, frames, n_raw, gpu.FRAMES_PIXELS, cfg, 0)
    assert p.one_launch == 1 and [ver[2 * f] for f in range(n)] == [1 if f == j else 0 for f in range(n)], ver
    assert all(ver[2 * f + 1] == 0 for f in range(n) if f != j), ver
    padded = np.zeros(2 * n_raw, ol.PIXEL_DT)
    for f in range(n):
        if f != j:
            padded[:n_px] = px[f]
            assert np.array_equal(out[f], padded.view(np.uint8))
    loop, lver = decode_loop(gpu, frames, n_raw, gpu.FRAMES_PIXELS, cfg)
    assert [lver[2 * f] for f in range(n)] == [ver[2 * f] for f in range(n)]


# ---- ticket re-arm: batched calls back to back ------------------------------------------------------------------------------------------
_B2B = [(2000, 334, 5), (1700, 334, 6)]          # (frames, pixels, seed): more tiles than two rounds of resident workgroups, so tickets are drawn


def _frames_back_to_back(t3):
    """Two batched encodes and two batched decodes of different batches queued on one stream with no synchronisation in between, then
    one synchronise -> [sha256 of batch A's coded frames, of B's, of A's decoded pixels, of B's, verdict sums]."""
    import torch
    cfg = t3.make_cfg(mode=1, **K20); s = stream()
    bat = []
    for n, n_px, seed in _B2B:
        px = frame_pixels(n, n_px, seed)
        pe = t3.frames_plan(False, n_px, n, cfg, t3.FRAMES_PIXELS); pd = t3.frames_plan(True, n_px, n, cfg, t3.FRAMES_PIXELS)
        d_in, a_in = to_dev([q.view(np.uint8) for q in px], pe.in_stride_min)
        d_cod, a_cod = dev_out(n, pe.out_stride_min); d_px, a_px = dev_out(n, pd.out_stride_min)
        ver = torch.full((2 * n,), 7, dtype=torch.int32, device="cuda")
        bat.append((n, n_px, pe, pd, d_in, a_in, d_cod, a_cod, d_px, a_px, ver))
    torch.cuda.synchronize()
    for n, n_px, pe, pd, d_in, a_in, d_cod, a_cod, d_px, a_px, ver in bat:
        t3.encode_frames_dev(a_in, n_px, t3.FRAMES_PIXELS, pe.in_stride_min, n, cfg, a_cod, pe.out_stride_min, s)
    for n, n_px, pe, pd, d_in, a_in, d_cod, a_cod, d_px, a_px, ver in bat:
        t3.decode_frames_async(a_cod, pe.out_bytes // 9, pe.out_stride_min, n, cfg, (n_px + 1) // 2, a_px, pd.out_stride_min, t3.FRAMES_PIXELS, ver.data_ptr(), s)
    torch.cuda.synchronize()
    res = []
    for i in (6, 8):                                                       # the coded frames of both batches, then their decoded pixels
        for b in bat:
            n, pe, pd = b[0], b[2], b[3]
            frames = split_out(b[i], n, pe.out_stride_min if i == 6 else pd.out_stride_min, pe.out_bytes if i == 6 else pd.out_bytes)
            res.append(hashlib.sha256(b"".join(f.tobytes() for f in frames)).hexdigest())
    res.append([int(b[-1].abs().sum().item()) for b in bat])
    return res


_B2B_CHILD = r"""
import json, os, sys
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import __graft_entry__ as ge
from test_gpu_frames import _frames_back_to_back
t3 = ge.load_package(); t3.init(0)
print("runs " + json.dumps(_frames_back_to_back(t3)))
"""


def test_frames_back_to_back(gpu, orc):
    """The ticket counters across batched launches: a launch's last workgroup re-arms them while the next launch is already queued.
    Both batches hold more tiles (one per frame) than two rounds of resident workgroups -- at most three 512-thread workgroups per
    compute unit in both kernels -- so tickets are drawn.  Once more with the static-tile fallback (T3HIP_STATIC_TILES=1, read once per
    process: a child of its own)."""
    import torch
    assert "T3HIP_STATIC_TILES" not in os.environ, "the launches must draw tile tickets"
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert all(n > 2 * 3 * cus for n, _, _ in _B2B), cus
    want = []
    for kind in ("coded", "pixels"):
        for n, n_px, seed in _B2B:
            px, coded = oracle_batch(n, n_px, 1, 2, seed)
            if kind == "coded":
                want.append(hashlib.sha256(b"".join(c.tobytes() for c in coded)).hexdigest())
            else:
                h = hashlib.sha256()
                for f in range(n):
                    rc, opx = orc.decode_frame(coded[f].reshape(-1, 9), ol.make_cfg(mode=1, **K20)); assert rc == 0
                    h.update(opx.tobytes())
                want.append(h.hexdigest())
    want.append([0, 0])
    got = _frames_back_to_back(gpu)
    assert got == want
    env = dict(os.environ, T3HIP_STATIC_TILES="1")
    r = subprocess.run([sys.executable, "-c", "ROOT = %r\n" % ROOT + _B2B_CHILD], env=env, capture_output=True, text=True, timeout=600)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("runs ")]
    assert r.returncode == 0 and lines, r.stdout[-2000:] + r.stderr[-4000:]
    assert json.loads(lines[0][len("runs "):]) == want


# ---- the per-frame path, arguments ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["p5_tile64_luma", "p2_beacon83", "raw_words"])
def test_per_frame_path(gpu, orc, name):
    """Framings the fused single-k kernels do not serve -- per-band k in 2-D, a beacon, raw words either way -- run as a loop of the
    single-frame entries inside the call: one_launch == 0, bytes and verdict words equal those entries' frame by frame, and the oracle's."""
    n, n_px = 3, 4861
    px = frame_pixels(n, n_px, 9)
    kw = K20 if name == "raw_words" else PER_FRAME[name]
    fmt = gpu.FRAMES_WORDS if name == "raw_words" else gpu.FRAMES_PIXELS
    cfg = gpu.make_cfg(mode=1, **kw); n_raw = (n_px + 1) // 2
    units = [orc.pack_pixels(q).reshape(-1) for q in px] if name == "raw_words" else [q.view(np.uint8) for q in px]
    n_units = n_raw if name == "raw_words" else n_px
    p, got = encode_batch(gpu, units, n_units, fmt, cfg, 4096 + 16)
    assert p.one_launch == 0 and p.tiles_per_frame == 0
    loop = encode_loop(gpu, units, n_units, fmt, cfg)
    for f in range(n):
        rc, w = orc.encode_frame(px[f], ol.make_cfg(mode=1, **kw)); assert rc == 0
        assert np.array_equal(got[f], np.ascontiguousarray(w).reshape(-1)) and np.array_equal(got[f], loop[f])
    L = gpu.plan(n_raw, cfg)
    dp, seen, out, ver = decode_batch(gpu, got, n_raw, fmt, cfg, 4096 + 16)
    assert dp.one_launch == 0 and ver == [0] * (2 * n), ver
    dloop, lver = decode_loop(gpu, got, n_raw, fmt, cfg)
    assert lver == ver and all(np.array_equal(a, b) for a, b in zip(out, dloop))
    padded = np.zeros(2 * n_raw, ol.PIXEL_DT)
    for f in range(n):
        padded[:n_px] = px[f]
        want = orc.pack_pixels(padded).reshape(-1) if name == "raw_words" else padded.view(np.uint8)
        assert np.array_equal(out[f], want)
    assert L.n_raw_words == n_raw


def test_frames_arguments(gpu):
    """A base that is not 16-byte aligned, a stride that is no multiple of 16 or below the plan's minimum: T3_E_ARG, whichever path the
    framing takes; the empty batch is T3_OK and launches nothing; one frame forwards to the single-frame entry (any stride)."""
    import torch
    n, n_px = 3, 4861
    for cfg in (gpu.make_cfg(mode=1, **K20), gpu.make_cfg(mode=1, **PER_FRAME["p2_beacon83"])):
        p = gpu.frames_plan(False, n_px, n, cfg, gpu.FRAMES_PIXELS); d = gpu.frames_plan(True, n_px, n, cfg, gpu.FRAMES_PIXELS)
        src = torch.zeros(n * p.in_stride_min + 64, dtype=torch.uint8, device="cuda"); cod = torch.zeros(n * p.out_stride_min + 64, dtype=torch.uint8, device="cuda")
        pix = torch.zeros(n * d.out_stride_min + 64, dtype=torch.uint8, device="cuda"); ver = torch.zeros(2 * n, dtype=torch.int32, device="cuda")
        bad_enc = [(8, 0, 0, 0), (0, 8, 0, 0), (0, 0, 8, 0), (0, 0, 0, 8), (0, 0, -16, 0), (0, 0, 0, -16)]        # (in base, out base, in stride, out stride) offsets
        for bi, bo, si, so in bad_enc:
            with pytest.raises(gpu.T3Error) as e:
                gpu.encode_frames_dev(src.data_ptr() + bi, n_px, gpu.FRAMES_PIXELS, p.in_stride_min + si, n, cfg, cod.data_ptr() + bo, p.out_stride_min + so, stream())
            assert e.value.code == gpu.E_ARG, (bi, bo, si, so)
            with pytest.raises(gpu.T3Error) as e:
                gpu.decode_frames_async(cod.data_ptr() + bi, p.out_bytes // 9, d.in_stride_min + si, n, cfg, (n_px + 1) // 2, pix.data_ptr() + bo, d.out_stride_min + so,
                                        gpu.FRAMES_PIXELS, ver.data_ptr(), stream())
            assert e.value.code == gpu.E_ARG, (bi, bo, si, so)
        assert gpu.encode_frames_dev(0, n_px, gpu.FRAMES_PIXELS, 0, 0, cfg, 0, 0, stream()) == p.out_bytes // 9          # the empty batch
        gpu.decode_frames_async(0, p.out_bytes // 9, 0, 0, cfg, (n_px + 1) // 2, 0, 0, gpu.FRAMES_PIXELS, 0, stream())
        torch.cuda.synchronize()
    with pytest.raises(gpu.T3Error) as e:
        gpu.frames_plan(False, n_px, 65536, gpu.make_cfg(mode=1, **K20))
    assert e.value.code == gpu.E_ARG


# ---- host entries, the C++ names ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_host_frames_round_trip(gpu, orc, mode):
    """encode_frames / decode_frames on host buffers: the coded frames are the oracle's; a frame with an uncorrectable block (FIXED) gets
    T3_E_RS in frame_rc and comes back empty, its neighbours T3_OK and their pixels; frame 0's header is remembered.  COMPAT: the
    reference's decoder refuses the header its own encoder writes (the header blocks are coded in the reference's arithmetic and checked
    as RS(26,18) codewords), so the round trip's frame_rc is the oracle's T3_E_HEADER for every frame; what decode_frames does with
    COMPAT streams that decoder takes is test_host_frames_compat_decode."""
    n, n_px, j = 4, 4861, 2
    px, want = oracle_batch(n, n_px, mode)
    ok, coded = gpu.encode_frames(px, gpu.make_cfg(mode=mode, **K20))
    assert ok and len(coded) == n and all(np.array_equal(c.reshape(-1), w) for c, w in zip(coded, want))
    padded = np.zeros(2 * ((n_px + 1) // 2), ol.PIXEL_DT)
    if mode == 0:
        orcs = [orc.decode_frame(c, ol.make_cfg(mode=0, **K20))[0] for c in coded]
        assert orcs == [gpu.E_HEADER] * n, orcs
        rcs, back = gpu.decode_frames(coded, gpu.DecoderContext(mode=0))
        assert rcs == orcs and all(len(b) == 0 for b in back), rcs
        assert [gpu.decode_frame(c, gpu.DecoderContext(mode=0))[0] for c in coded] == [False] * n
        with pytest.raises(ValueError):
            gpu.encode_frames([px[0], px[1][:-1]], gpu.make_cfg(mode=mode, **K20))
        return
    if mode == 1:
        L = gpu.plan((n_px + 1) // 2, gpu.make_cfg(mode=1, **K20)); o = L.header_syms + L.band_body_off[2] + 26 * 7
        for add in range(1, 27):
            cand = want[j].copy(); cand[o: o + 5] = (cand[o: o + 5] + add) % 27
            if orc.decode_frame(cand.reshape(-1, 9), ol.make_cfg(mode=1, **K20))[0] == gpu.E_RS:
                coded[j] = cand.reshape(-1, 9); break
        else:
            pytest.fail("the oracle accepted every pattern")
    dctx = gpu.DecoderContext(mode=mode)
    rcs, back = gpu.decode_frames(coded, dctx)
    assert rcs == [gpu.E_RS if (mode == 1 and f == j) else gpu.OK for f in range(n)], rcs
    assert dctx.cfg_last_seen.profile == 2
    for f in range(n):
        if rcs[f] != gpu.OK:
            assert len(back[f]) == 0
            continue
        rc, opx = orc.decode_frame(coded[f], ol.make_cfg(mode=mode, **K20)); assert rc == 0
        assert np.array_equal(back[f].view(np.uint8), opx.view(np.uint8))
        if mode == 1:
            padded[:n_px] = px[f]
            assert np.array_equal(back[f].view(np.uint8), padded.view(np.uint8))
    with pytest.raises(ValueError):
        gpu.encode_frames([px[0], px[1][:-1]], gpu.make_cfg(mode=mode, **K20))


def test_host_frames_compat_decode(gpu, orc):
    """decode_frames, COMPAT flavour (the per-frame path): equal-sized streams laid out as the reference's decoder reads them, frame j
    with up to 5 symbol errors in some blocks.  Every frame's code and pixels are the oracle's decode_frame of that frame, whatever it
    says of frame j; frame 0's header is remembered as the oracle remembers it."""
    from test_oracle_vs_ref import decoder_consistent_stream
    n, j, nbw = 4, 2, 600
    rng = np.random.default_rng(4242)
    ocfg = ol.make_cfg(mode=0, **K20)
    streams = [decoder_consistent_stream(orc, rng, ocfg, nbw, 5 if f == j else 0) for f in range(n)]
    want = []
    for s in streams:
        oseen = ol.make_cfg(mode=0)
        want.append(orc.decode_frame(s, oseen) + (oseen,))
    assert want[0][0] == gpu.OK and all(w[0] in (gpu.OK, gpu.E_RS) for w in want), [w[0] for w in want]
    dctx = gpu.DecoderContext(mode=0)
    rcs, back = gpu.decode_frames(streams, dctx)
    assert rcs == [w[0] for w in want], rcs
    a, b = dctx.cfg_last_seen.as_dict(), want[0][2].as_dict()
    assert {k: v for k, v in a.items() if k != "mode"} == {k: v for k, v in b.items() if k != "mode"}
    for f in range(n):
        if rcs[f] != gpu.OK:
            assert len(back[f]) == 0
            continue
        assert np.array_equal(back[f].view(np.uint8), want[f][1].view(np.uint8))
        ok, one = gpu.decode_frame(streams[f], gpu.DecoderContext(mode=0))            # ... and the single-frame entry's
        assert ok and np.array_equal(one.view(np.uint8), back[f].view(np.uint8))


def test_frames_demo(gpu, orc, tmp_path):
    """tests/cpp/frames_demo.cpp: encode_frames / decode_frames of include/ternary_codec_v6.hpp over vectors of frames, FIXED RS(26,20),
    frame 1 of 3 damaged before the decode."""
    lib = os.path.join(ROOT, "ternary-image-codec_amd"); exe = os.path.join(str(tmp_path), "frames_demo")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include", "compat"), "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "frames_demo.cpp"), "-L" + lib, "-lt3hip", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-o", exe], check=True)
    n, n_px, bad = 3, 4861, 1
    px, want = oracle_batch(n, n_px, 1)
    p = lambda name: os.path.join(str(tmp_path), name)
    np.concatenate(px).tofile(p("in.px"))
    r = subprocess.run([exe, str(n), str(n_px), "1", str(bad), p("in.px"), p("words"), p("px")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    info = json.loads(r.stdout.strip().splitlines()[-1])
    assert np.array_equal(np.fromfile(p("words"), np.uint8), np.concatenate(want))
    dead = want[bad].copy(); hs = 90; dead[hs: hs + 13] = (dead[hs: hs + 13] + 1) % 27
    rc_dead, _ = orc.decode_frame(dead.reshape(-1, 9), ol.make_cfg(mode=1, **K20))
    assert info["frames"] == n and info["words"] == len(want[0]) // 9 and info["uneven_refused"] == 1 and info["seen_profile"] == 2
    assert info["good"] == [0 if (f == bad and rc_dead != 0) else 1 for f in range(n)] and info["all"] == (1 if rc_dead == 0 else 0)
    back = np.fromfile(p("px"), ol.PIXEL_DT).reshape(n, -1)
    for f in range(n):
        if info["good"][f]:
            src = dead if f == bad else want[f]
            rc, opx = orc.decode_frame(src.reshape(-1, 9), ol.make_cfg(mode=1, **K20)); assert rc == 0
            assert np.array_equal(back[f], opx)
