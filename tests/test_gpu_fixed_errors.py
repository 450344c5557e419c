"""GPU tests of the FIXED (v6c) frame decoders over the full error range.  Every frame decoder carries a corrector of its own (fx2_single /
fx2_correct in the fused and one-launch UEP kernels, fx_correct in the two-kernel decoder, rs_correct in the generic one); these tests feed
each of them, through every entry point, streams built by tests/rs_patterns.py:

  <= t     every band at its OWN t: every single error (26 positions x 26 values), every position pair, every value pair, >= 2000 seeded
           sets per higher weight, t errors in block 0 of band 0 (positions 0 and 1) and in every band's last (padded) block.  From block
           703 on every block of every band carries >= 2 errors: whole tiles of queue-bound blocks.  Expected: the input itself.
  near     >= 200 blocks per code beyond t that lie within t of ANOTHER codeword, the rest clean: accepted, decoded to that codeword (the
           oracle's output, which tests/test_fixed_rs_semantics.py proves to be that codeword), different from the original.
  far      M blocks with no codeword within t (among them rows with syndromes (s, 0, .., 0)) on top of the <= t schedule: the verdict counts
           exactly M, the synchronous entries refuse the frame, and in the one-k 1-D framing every pixel tile without a far block still
           decodes to the original.

Which decoder a framing reaches is read from the plan_fixed_* functions of t3_dec_plan.cpp: one k, 1-D (with or without a beacon of
period >= 2) -> fused kernel; pixels out of at most two codes and / or a 2-D interleave whose rows are a multiple of 4 symbols -> one-launch
UEP kernel; everything else (raw words of those framings, four codes, 7 x 5 tiles) -> two-kernel decoder; T3HIP_TWO_KERNEL_DECODE /
T3HIP_GENERIC_DECODE force the two-kernel / generic path.  All expectations are proven on the CPU in test_fixed_rs_semantics.py (B4)."""
import functools
import os

import numpy as np
import pytest

import oracle_lib as ol
import rs_patterns as rp

pytestmark = pytest.mark.gpu

# configuration -> the outputs checked (True: pixels, False: raw 26-trit words)
OUTPUTS = {
    "k24": (True, False), "k22": (True, False), "k20": (True, False), "k18": (True, False),
    "k22_beacon2_slot8": (True,), "k20_beacon83": (True,),
    "luma": (True, False), "uep_18_22": (True, False), "uep_20_24": (True, False),
    "four_codes": (True, False),
    "2d_64x64_k20": (True,), "2d_luma_1024x16": (True,), "2d_7x5_k22": (True,),
}
assert set(OUTPUTS) == set(rp.CONFIGS)
KNOBS = [("T3HIP_GENERIC_DECODE", "k18"), ("T3HIP_GENERIC_DECODE", "luma"), ("T3HIP_TWO_KERNEL_DECODE", "luma"), ("T3HIP_TWO_KERNEL_DECODE", "2d_64x64_k20")]


@functools.lru_cache(maxsize=4)
def _frame(name, what):
    import __graft_entry__ as ge
    t3 = ge.load_package()
    cfg = t3.make_cfg(mode=1, **rp.CONFIGS[name])
    return rp.make_frame(ol.oracle(), lambda n_raw: t3.plan(n_raw, cfg), name, what)


class Dev:
    """One frame's buffers on the device and the two device entry points."""

    def __init__(self, gpu, fr):
        import torch
        self.t, self.gpu, self.fr = torch, gpu, fr
        self.cfg = gpu.make_cfg(mode=1, **fr.kw)
        self.n_px = len(fr.padded)
        self.s = torch.cuda.current_stream().cuda_stream
        self.out = torch.zeros(self.n_px * 6 + 64, dtype=torch.uint8, device="cuda")
        self.ver = torch.full((2,), 7, dtype=torch.int32, device="cuda")

    def upload(self, stream):
        return self.t.from_numpy(np.ascontiguousarray(stream).reshape(-1)).cuda()

    def units(self, to_pixels):
        return (self.n_px, 6) if to_pixels else (self.fr.n_raw, 9)

    def run_async(self, d, to_pixels):
        n, sz = self.units(to_pixels)
        self.out.fill_(0xA5); self.ver.fill_(7)
        got = self.gpu.decode_frame_async(d.data_ptr(), d.numel() // 9, self.cfg, self.fr.n_raw, self.out.data_ptr(), n, self.ver.data_ptr(), to_pixels, self.s)
        self.t.cuda.synchronize()
        assert got == n
        return self.ver.cpu().tolist(), self.out[: n * sz].cpu().numpy()

    def run_sync(self, d, to_pixels):
        n, sz = self.units(to_pixels)
        self.out.fill_(0xA5)
        seen = self.gpu.DecoderContext(mode=1).cfg_last_seen
        rc, got = self.gpu.decode_profile_dev(d.data_ptr(), d.numel() // 9, seen, self.out.data_ptr(), n, to_pixels, self.s)
        self.t.cuda.synchronize()
        return rc, got, self.out[: n * sz].cpu().numpy()


def expected(orc, fr, case, stream):
    """-> {to_pixels: bytes} the decoders must give (None: the frame is refused)."""
    if case == "sched":
        px = fr.padded
    elif case == "near":
        rc, px = orc.decode_frame(stream, ol.make_cfg(mode=1))
        assert rc == 0 and len(px) == len(fr.padded) and not np.array_equal(px, fr.padded)
    else:
        return None
    return {True: px.view(np.uint8).reshape(-1), False: np.asarray(orc.pack_pixels(px)).reshape(-1)}


def check_streams(gpu, dev, fr, streams, outputs, what, label):
    """streams: (case, the stream on the device, M far rows in it, where they are, expected(...)) -- both device entries, every output."""
    for case, d, M, where, want in streams:
        for to_pixels in outputs:
            ver, got = dev.run_async(d, to_pixels)
            assert ver == [0, M], (label, what, case, to_pixels, ver)
            rc, n, got_s = dev.run_sync(d, to_pixels)
            if want is None:
                assert rc == gpu.E_RS, (label, what, case, to_pixels, rc)
                if to_pixels and fr.name in rp.ONE_K and what != "small":     # tiles are independent: the rest of the frame still decodes
                    keep = rp.pixels_outside_tiles(dev.n_px, fr.ks[0], rp.far_tiles_one_k(fr.ks[0], where))
                    assert keep.any()
                    assert np.array_equal(got.view(ol.PIXEL_DT)[keep], fr.padded[keep]), (label, what, case)
            else:
                assert np.array_equal(got, want[to_pixels]), (label, what, case, to_pixels, "async")
                assert rc == 0 and n == dev.units(to_pixels)[0] and np.array_equal(got_s, want[to_pixels]), (label, what, case, to_pixels, "sync")


def check_device_entries(gpu, orc, fr, outputs, what, label):
    dev = Dev(gpu, fr)

    def streams():
        for case in rp.CASES[what]:
            stream, M, where = fr.stream(case)
            yield case, dev.upload(stream), M, where, expected(orc, fr, case, stream)
    check_streams(gpu, dev, fr, streams(), outputs, what, label)


@pytest.mark.parametrize("what", sorted(rp.CASES))
@pytest.mark.parametrize("name", sorted(rp.CONFIGS))
def test_fixed_frame_decoders_full_error_range(gpu, orc, name, what):
    """Every framing of the table above through t3hip_decode_frame_async and t3hip_decode_profile_dev, pixels and (where listed) raw words,
    at three sizes: every band holds the whole schedule ('full'; one k: >= 66 tiles), the same with an odd pixel count and the last block of
    every band zero-padded ('padded'), and under one tile ('small').  Coverage of the schedule is asserted per band for the two large sizes."""
    fr = _frame(name, what)
    if what != "small":
        for b, rec in enumerate(fr.sched()[1]):
            rp.assert_coverage(fr.ks[b], rec)                  # no band below its own t, all 676 single errors, all 325 pairs
    check_device_entries(gpu, orc, fr, OUTPUTS[name], what, name)


@pytest.mark.parametrize("knob,name", KNOBS)
def test_fixed_frame_decoders_forced_paths(gpu, orc, knob, name):
    """The same frames with the two-kernel decoder (fx_correct) and the generic gather decoder (rs_correct) forced by their knobs."""
    os.environ[knob] = "1"
    try:
        check_device_entries(gpu, orc, _frame(name, "full"), (True,), "full", "%s %s" % (knob, name))
    finally:
        os.environ.pop(knob, None)


@pytest.mark.parametrize("name", rp.ONE_K)
def test_fixed_other_entry_points(gpu, orc, name):
    """One k, 1-D: the window decode over the whole frame (tile-range path, pixels and RGB), the RGB entry and the host-buffer entry, which
    decodes a frame of this size chunk by chunk (>= 64 decoder tiles)."""
    import torch
    fr = _frame(name, "full")
    dev = Dev(gpu, fr); n = dev.n_px; s = dev.s
    assert -(-max(fr.blocks) // 52) >= 64
    rgb = torch.zeros(3 * n + 64, dtype=torch.uint8, device="cuda")
    for case in rp.CASES["full"]:
        stream, M, where = fr.stream(case)
        want = expected(orc, fr, case, stream)
        d = dev.upload(stream)
        for fmt, size in ((gpu.WINDOW_PIXELS, 6), (gpu.WINDOW_RGB, 3)):
            dev.out.fill_(0xA5); dev.ver.fill_(7)
            gpu.decode_window_async(d.data_ptr(), d.numel() // 9, dev.cfg, fr.n_raw, n, 1, 0, 0, n, 1, dev.out.data_ptr(), fmt, dev.ver.data_ptr(), s)
            torch.cuda.synchronize()
            assert dev.ver.cpu().tolist() == [0, M], (name, case, fmt)
            if want is not None:
                px = want[True].view(ol.PIXEL_DT)
                assert np.array_equal(dev.out[: n * size].cpu().numpy(), want[True] if size == 6 else orc.quant_to_rgb(px)), (name, case, fmt)
        rgb.fill_(0xA5); dev.ver.fill_(7)
        gpu.decode_rgb_async(d.data_ptr(), d.numel() // 9, dev.cfg, n, rgb.data_ptr(), dev.ver.data_ptr(), s)
        torch.cuda.synchronize()
        assert dev.ver.cpu().tolist() == [0, M], (name, case, "rgb")
        if want is not None:
            assert np.array_equal(rgb[: 3 * n].cpu().numpy(), orc.quant_to_rgb(want[True].view(ol.PIXEL_DT))), (name, case, "rgb")
        ok, back = gpu.decode_frame(stream, gpu.DecoderContext(mode=1))
        if want is None:
            assert not ok and len(back) == 0, (name, case, "host")
        else:
            assert ok and np.array_equal(np.asarray(back).view(np.uint8).reshape(-1), want[True]), (name, case, "host")
