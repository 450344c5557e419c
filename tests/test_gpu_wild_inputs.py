"""Every encoder front end on LONE out-of-range input values, and on every input value there is.

The converters of csrc/t3_enc_convert.h run a fast path for in-range input and an exact reduction (red_y, red_c, mod27) behind a
wave-uniform ballot.  The suite's other wild frames are wild all over -- test_gpu_parity.rand_pixels(in_range=False), frame_ends.WILD_EVERY,
the words of test_gpu_scrambler -- so every wave takes the reduction and the fast path never meets a wild value.  Here it does: in the
frames of tests/wild_inputs.py a wild value is the only one of its wave.  Every comparison is byte for byte with the CPU oracle's stream
(oracle_lib: encode_frame, encode_profile, pack_pixels), computed once per sweep and uploaded once; the streams are compared on the
device, the first differing (frame, byte) is reported.  tests/test_wild_inputs_lattice.py proves on the CPU what the frames hold and
that the oracle's stream of every frame changes when the reduction is missed.

P = 769 (wild_inputs.P): the wild values of a frame lie 769 units apart.  One ballot covers one loop step of one wave, and the longest run of
consecutive input units a wave takes in one step is 64 lanes x 4 triples x 3 = 768 pixels (convert_pixels_packed) or 768 words
(convert_words_half, whose 56 tested bytes reach two bytes into the other half of the same lane unit); convert_groups stays within 384.
Two values 769 apart never share a ballot wherever a wave's lane units are consecutive: 1-D, and the 2-D flows that stage whole rows.

Frame s of sweep c holds a wild value at every unit s + j P -- component (c + j) % 3 of the pixel, byte (w + c) % 9 of the word -- so the 3 P
pixel frames make every (pixel, component) wild once and the 9 P word frames every (word, byte): every slot of a lane unit (twelve pixels x
three components, low and high half of the packed registers; twelve words x nine bytes), every lane, the first and last unit of every tile
and a last unit with 1, 2, 3 or 4 live triples (liveA / liveB) are reached by construction.  The value cycles with the lane unit and with j,
so that every listed edge value meets each of those slots as well (counted by the lattice test): a range check that gets one edge wrong in
one half or one pair of registers meets that edge there, alone.  No planner is asked where a tile ends; the base
frames are long enough for two tile boundaries and a ragged, odd end (the lattice test holds them against tests/golden/enc_plan.json).

Conversion paths of encode_body (t3_encode.h; kernel and tile picked by plan_encode / t3_enc_plan.cpp) and the configuration that reaches each:
  full sweeps, RS(26,20) 1-D FIXED
    pixels   encode_kernel_k<FE_PIXELS, 0, 6>: convert_pixels_packed<4, FE_PIXELS, false>, stores of whole lane units
             the same frames in one launch of enc_frames_k<FE_PIXELS, 6> (t3hip_encode_frames_dev): the tile space of all frames
    words    encode_kernel_k<FE_WORDS, 0, 6>: convert_words_packed -> convert_words_half<2, 0 | 1>
  thinned sweeps (sweep 0: every unit wild once, the components cycling), pixels | raw words
    k20_compat            RS(26,20) 1-D COMPAT: the two converters above under the reference's framing (a band's tail dropped: other ragged ends)
    luma                  encode_kernel_uep<FE, 0>: the same converters in front of the grouped phase 2 (other tiles: 7920 | 9900 symbols)
    four_codes            no tile serves four codes at once: two launches of encode_kernel_uep, one per pair of codes, each converting the
                          whole frame (the dispatch never gives four codes to encode_kernel_mixed); the larger base frame
    k20_beacon83          encode_kernel_k<FE, 0, 6, BCN = true>: the beacon in the stores, the converters unchanged
    2d_64x64_luma         IL = 1, rows staged whole: convert_pixels_packed<4, FE_PIXELS, false> from the tile's first row on, then
                          reverse_rows16 | raw words: the row-by-row flow, convert_groups<FE_WORDS, true, 2> (its `bad` ballot per triple)
    2d_1024x16_k20        IL = 2, the run-placed flow (`placed`): convert_pixels_packed<4, FE_PIXELS, true> over up to three runs, whole lane
                          units and dword stores at a run's ends, reverse_rows_placed; the stream's last tile through the dword cursor flow
    2d_513x8_k20          IL = 2 with rows that are no multiple of 4: convert_pixels_packed's symbol-by-symbol stores
    2d_7x5_k22            IL = 1, narrow rows: whole-unit stores in pre-interleave order, permute_rows moves symbol by symbol
    2d_512x8_three_codes  the one place the dispatch picks encode_kernel_mixed (three codes, 2-D rows of 512 and more, pixel input: no UEP tile
                          fits; 704 threads, tile 14256): convert_pixels_packed<8, FE_PIXELS, false>, symbols pre-scaled by 8
    raw words in 2-D (all five 2-D configurations): convert_groups<FE_WORDS, true, 2>
  exhaustive frames (dense: they pin red_y, red_c, mod27 over their whole domain on the device)
    t3hip_pack_pixels_dev / t3hip_unpack_words_dev (the RAW packer reduces without a ballot), RS(26,20) 1-D and 2-D 64 x 64 from pixels and words
In the run-placed flow a wave that straddles two runs of a tile spans the gap between them and may meet two wild values; everywhere else
each wild value is alone in its ballot.

Round trip: the stream the device encodes of every 50th frame of the pixel sweep decodes (t3hip_decode_frame_async) to the oracle's
unpack_words(pack_pixels(frame)).

Time on an MI355X (measured): the module in 13 s; a full sweep of 3 P frames 0.9 - 1.3 s plus 1.6 s once for the pixel sweep's oracle streams, a
thinned sweep 0.2 - 0.6 s, the exhaustive frames 0.1 - 0.25 s each."""
import numpy as np
import pytest

import bounds
import oracle_lib as ol
import rs_patterns as rp
import wild_inputs as wi

pytestmark = pytest.mark.gpu

K20 = wi.K20
FILL, TAIL = 0xA5, 64                             # guard bytes behind every frame's coded words
ROUND_TRIP_EVERY = 50
THINNED = wi.THINNED                              # (the launches listed there are held to the planner by tests/test_wild_inputs_lattice.py)


def st():
    import torch
    return torch.cuda.current_stream().cuda_stream


def r16(x):
    return (x + 15) & ~15


def entry(gpu, front_end):
    return gpu.encode_frame_dev if front_end == "pixels" else gpu.encode_profile_dev


def up(a):
    import torch
    return torch.from_numpy(np.array(a, copy=True)).cuda()


def upload_frames(inputs, stride):
    """(frames, bytes) host array -> device tensor (frames, stride), the rest of every stride filled."""
    import torch
    buf = np.full((inputs.shape[0], stride), FILL, np.uint8)
    buf[:, : inputs.shape[1]] = inputs
    return torch.from_numpy(buf).cuda()


def compare(d_out, d_want, label, name_of):
    """Every frame's coded bytes against the expected ones, the bytes behind them against the fill; on the device."""
    import torch
    used = d_want.shape[1]
    got = d_out[:, :used]
    if not torch.equal(got, d_want):
        ne = got != d_want
        frames = torch.nonzero(ne.any(dim=1)).flatten()
        f = int(frames[0]); b = int(torch.nonzero(ne[f]).flatten()[0])
        raise AssertionError("%s: %d of %d frames differ from the oracle's stream; first: frame %d %s, byte %d (got %d, expected %d, %d bytes of it differ)"
                             % (label, len(frames), len(d_want), f, name_of(f), b, int(got[f, b]), int(d_want[f, b]), int(ne[f].sum())))
    tail = d_out[:, used:] != FILL
    assert not bool(tail.any()), "%s: bytes behind the coded words were written, first in frame %d" % (label, int(torch.nonzero(tail.any(dim=1)).flatten()[0]))


def run_single(gpu, sw, cfg, label):
    """Every frame of the sweep through the single-frame device entry of its front end, one call each, into one output tensor."""
    import torch
    used = sw.want.shape[1]; cap = used // 9
    assert used == 9 * gpu.encoded_words(sw.W, cfg), label
    in_stride, out_stride = r16(sw.inputs.shape[1]), r16(used) + TAIL
    d_in = upload_frames(sw.inputs, in_stride)
    d_out = torch.full((len(sw), out_stride), FILL, dtype=torch.uint8, device="cuda")
    d_want = up(sw.want)
    fn, a_in, a_out, s = entry(gpu, sw.front_end), d_in.data_ptr(), d_out.data_ptr(), st()
    for f in range(len(sw)):
        n = fn(a_in + f * in_stride, sw.n_units, cfg, a_out + f * out_stride, cap, s)
        assert n == cap, (label, f, n, cap)
    bounds.sync()
    compare(d_out, d_want, label, lambda f: "(sweep %d, s = %d)" % sw.index[f])
    assert np.array_equal(d_in[:, : sw.inputs.shape[1]].cpu().numpy(), sw.inputs), "%s: the input was written" % (label,)


def cs_id(cs):
    return "sweeps_" + "".join(str(c) for c in cs)


# ---- full sweeps: RS(26,20), 1-D, FIXED ------------------------------------------------------------------------------------------------------
def test_lone_pixels_full_sweep(gpu, orc):
    """t3hip_encode_frame_dev on the 3 P frames: every (pixel, component) of the frame wild once, alone in its wave."""
    sw = wi.sweep("pixels", K20, 1)
    assert len(sw) == 3 * wi.P
    run_single(gpu, sw, gpu.make_cfg(mode=1, **K20), "pixels, RS(26,20) FIXED")


def test_lone_pixels_full_sweep_batched(gpu, orc):
    """The same 3 P pixel frames through t3hip_encode_frames_dev at the plan's minimal strides: ONE launch of enc_frames_k, in whose tile
    space a frame's last tile is followed by the next frame's first."""
    import torch
    sw = wi.sweep("pixels", K20, 1)
    cfg = gpu.make_cfg(mode=1, **K20)
    p = gpu.frames_plan(False, sw.n_units, len(sw), cfg, gpu.FRAMES_PIXELS)
    assert p.one_launch == 1 and p.n_frames == len(sw) <= 65535 and p.tiles_per_frame >= 3
    assert p.in_bytes == sw.inputs.shape[1] and p.out_bytes == sw.want.shape[1]
    ins, outs = p.in_stride_min, p.out_stride_min
    d_in = upload_frames(sw.inputs, ins)
    d_out = torch.full((len(sw) * outs + TAIL,), FILL, dtype=torch.uint8, device="cuda")
    words = gpu.encode_frames_dev(d_in.data_ptr(), sw.n_units, gpu.FRAMES_PIXELS, ins, len(sw), cfg, d_out.data_ptr(), outs, st())
    bounds.sync()
    assert 9 * words == p.out_bytes
    assert bool((d_out[len(sw) * outs:] == FILL).all()), "bytes behind the last frame's stride were written"
    compare(d_out[: len(sw) * outs].view(len(sw), outs), up(sw.want), "pixels, RS(26,20) FIXED, one batched launch", lambda f: "(sweep %d, s = %d)" % sw.index[f])


def test_lone_pixel_streams_decode_to_the_reduced_frames(gpu, orc):
    """Round trip on the device: every 50th frame of the pixel sweep through t3hip_encode_frame_dev, and the stream it wrote through
    t3hip_decode_frame_async: the pixels the reference's packer makes of the frame -- unpack_words(pack_pixels(frame)), the wild values
    reduced, the pad pixel behind -- with verdict [0, 0]."""
    import torch
    sw = wi.sweep("pixels", K20, 1)
    cfg = gpu.make_cfg(mode=1, **K20)
    used = sw.want.shape[1]; cap = used // 9
    coded = torch.empty(r16(used) + TAIL, dtype=torch.uint8, device="cuda")
    out = torch.empty(12 * sw.W + TAIL, dtype=torch.uint8, device="cuda")
    ver = torch.empty(2, dtype=torch.int32, device="cuda")
    for f in range(0, len(sw), ROUND_TRIP_EVERY):
        c, s = sw.index[f]
        px = wi.pixel_frame(sw.W, c, s)
        assert np.array_equal(wi.u8(px), sw.inputs[f])
        d = up(sw.inputs[f])
        coded.fill_(FILL); out.fill_(FILL); ver.fill_(7)
        assert gpu.encode_frame_dev(d.data_ptr(), sw.n_units, cfg, coded.data_ptr(), cap, st()) == cap
        n = gpu.decode_frame_async(coded.data_ptr(), cap, cfg, sw.W, out.data_ptr(), 2 * sw.W, ver.data_ptr(), True, st())
        bounds.sync()
        want = wi.u8(orc.unpack_words(orc.pack_pixels(px)))
        got = out.cpu().numpy()
        assert n == 2 * sw.W and ver.cpu().tolist() == [0, 0], (sw.index[f], n, ver.cpu().tolist())
        assert np.array_equal(got[: 12 * sw.W], want) and (got[12 * sw.W:] == FILL).all(), sw.index[f]


@pytest.mark.parametrize("cs", [wi.WORD_SWEEPS[i: i + 3] for i in range(0, 9, 3)], ids=cs_id)
def test_lone_words_full_sweep(gpu, orc, cs):
    """t3hip_encode_profile_dev, 3 P frames per case: sweeps 0, 1, 2 reach each of the 12 x 9 byte slots of a lane unit, the nine together
    make every (word, byte) of the frame wild once."""
    sw = wi.sweep("words", K20, 1, cs=cs)
    assert len(sw) == 3 * wi.P
    run_single(gpu, sw, gpu.make_cfg(mode=1, **K20), "raw words, RS(26,20) FIXED, sweeps %s" % (cs,))


# ---- thinned sweeps: the other conversion paths ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("front_end", ["pixels", "words"])
@pytest.mark.parametrize("name", list(THINNED))
def test_lone_values_thinned_sweep(gpu, orc, name, front_end):
    """The P frames of sweep 0 through the configuration's kernels (the module's docstring names the conversion path of each)."""
    kw, mode, W = THINNED[name][:3]
    sw = wi.sweep(front_end, kw, mode, W=W, cs=(0,))
    assert len(sw) == wi.P
    run_single(gpu, sw, gpu.make_cfg(mode=mode, **kw), "%s, %s" % (name, front_end))


# ---- exhaustive frames -----------------------------------------------------------------------------------------------------------------------
EXHAUSTIVE = {"k20": K20, "2d_64x64_k20": rp.CONFIGS["2d_64x64_k20"]}


def run_one(gpu, fn, data, n_units, cfg, want, label):
    import torch
    cap = len(want) // 9
    d_in = up(wi.u8(data))
    d_out = torch.full((len(want) + TAIL,), FILL, dtype=torch.uint8, device="cuda")
    n = fn(d_in.data_ptr(), n_units, cfg, d_out.data_ptr(), cap, st())
    bounds.sync()
    assert n == cap, (label, n, cap)
    compare(d_out.view(1, -1), up(want).view(1, -1), label, lambda f: "")


@pytest.mark.parametrize("name", list(EXHAUSTIVE))
def test_every_pixel_value_through_the_encoders(gpu, orc, name):
    """Every Yq, Cbq and Crq of the 16-bit domain in each pixel slot of a triple (dense: every wave reduces): red_y and red_c as the compiler
    built them, against the oracle."""
    px = wi.exhaustive_pixels()
    want = wi.encode("pixels", px, ol.make_cfg(mode=1, **EXHAUSTIVE[name]))
    run_one(gpu, gpu.encode_frame_dev, px, len(px), gpu.make_cfg(mode=1, **EXHAUSTIVE[name]), want, "every pixel value, %s" % name)


@pytest.mark.parametrize("name", list(EXHAUSTIVE))
def test_every_byte_value_through_the_encoders(gpu, orc, name):
    """Every byte value 0 .. 255 in each of the 108 byte slots of a lane unit of raw words."""
    raw = wi.exhaustive_words()
    want = wi.encode("words", raw, ol.make_cfg(mode=1, **EXHAUSTIVE[name]))
    run_one(gpu, gpu.encode_profile_dev, raw, len(raw), gpu.make_cfg(mode=1, **EXHAUSTIVE[name]), want, "every byte value, %s" % name)


def test_every_value_through_the_raw_packer(gpu, orc):
    """t3hip_pack_pixels_dev on the exhaustive pixel frame (the closed forms Y % 243, ((C + 40) mod 2^32) % 81, which the lattice test holds the
    oracle to), t3hip_unpack_words_dev on the exhaustive word frame."""
    import torch
    px = wi.exhaustive_pixels()
    want = wi.u8(orc.pack_pixels(px))
    assert np.array_equal(want, wi.u8(wi.words_of_components(wi.reduced_components(px))))
    d_px = up(wi.u8(px))
    d_words = torch.full((len(want) + TAIL,), FILL, dtype=torch.uint8, device="cuda")
    gpu.pack_pixels_dev(d_px.data_ptr(), len(px), d_words.data_ptr(), st())
    bounds.sync()
    compare(d_words.view(1, -1), up(want).view(1, -1), "t3hip_pack_pixels_dev, every pixel value", lambda f: "")
    raw = wi.exhaustive_words()
    want = wi.u8(orc.unpack_words(raw))
    d_raw = up(wi.u8(raw))
    d_out = torch.full((len(want) + TAIL,), FILL, dtype=torch.uint8, device="cuda")
    gpu.unpack_words_dev(d_raw.data_ptr(), len(raw), d_out.data_ptr(), st())
    bounds.sync()
    compare(d_out.view(1, -1), up(want).view(1, -1), "t3hip_unpack_words_dev, every byte value", lambda f: "")
