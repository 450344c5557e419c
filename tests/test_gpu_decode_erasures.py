"""GPU tests of the decode with erasures (include/t3hip.h, "decode with erasures"): decode_era_px_kernel<R, RGB, BCN> (path 1) and the
private copy + erasure repair + plain decoder (path 0) against expected_erasures of tests/erasure_patterns.py -- built on
rs_patterns.Field and the oracle only, proven on the CPU in tests/test_erasure_semantics.py -- and the oracle's decoder.  The input sits
in a guarded buffer that NO byte of may change (tests/bounds.py), the output in a guarded buffer of exactly the units the plan names.
Byte work: every comparison is exact."""
import functools

import numpy as np
import pytest

import bounds
import erasure_patterns as ep
import oracle_lib as ol
import rs_patterns as rp
from test_decode_erasures_plan import FUSED
from test_gpu_fixed_errors import OUTPUTS

pytestmark = pytest.mark.gpu
FILL = bounds.FILLS[0]
WORDS, PIXELS, RGB = 0, 1, 2
SIZE = {WORDS: 9, PIXELS: 6, RGB: 3}
SEED = {"small": 41, "padded": 42}


def formats(name):
    """the formats a configuration's decoders produce: OUTPUTS of test_gpu_fixed_errors.py, plus RGB where pixels are"""
    return tuple(f for to_px in OUTPUTS[name] for f in ((PIXELS, RGB) if to_px else (WORDS,)))


@functools.lru_cache(maxsize=4)
def _frame(name, what):
    import __graft_entry__ as ge
    t3 = ge.load_package()
    cfg = t3.make_cfg(mode=1, **rp.CONFIGS[name])
    return rp.make_frame(ol.oracle(), lambda n_raw: t3.plan(n_raw, cfg), name, what)


def want_bytes(orc, px, fmt):
    """`px` (PIXEL_DT, the pad pixel included) in the bytes of a format"""
    px = np.ascontiguousarray(px)
    if fmt == PIXELS:
        return px.view(np.uint8).reshape(-1)
    if fmt == WORDS:
        return np.asarray(orc.pack_pixels(px)).reshape(-1)
    return np.asarray(orc.quant_to_rgb(px)).reshape(-1)


def run(gpu, fr, stream, fmt, offset=0, fill=FILL):
    """One call on a guarded copy of `stream` that must come back byte-identical -> (the output's bytes, the four words)"""
    import torch
    b = np.ascontiguousarray(stream, np.uint8).reshape(-1)
    units = fr.n_raw if fmt == WORDS else 2 * fr.n_raw
    inb = bounds.Buf(len(b), fill, offset, data=b, name="coded frame")          # no may_change range: read-only
    out = bounds.Buf(units * SIZE[fmt], fill, 0, name="output")
    ver = torch.full((8,), 7, dtype=torch.int32, device="cuda")
    cfg = gpu.make_cfg(mode=1, **fr.kw)
    n = gpu.decode_erasures_frame_async(inb.ptr, len(b) // 9, cfg, fr.n_raw, out.ptr, units, fmt, ver.data_ptr(), torch.cuda.current_stream().cuda_stream)
    bounds.sync()
    v = ver.cpu().tolist()
    assert n == units and v[4:] == [7] * 4, ("units, or words behind the verdict were written", n, v)
    inb.result()                                                            # the input byte-identical, its guards intact
    return out.result(), v[:4]


def plain(gpu, fr, stream, fmt):
    """t3hip_decode_frame_async / t3hip_decode_rgb_async on `stream` -> (bytes, the two words)"""
    import torch
    d = torch.from_numpy(np.ascontiguousarray(stream, np.uint8).reshape(-1).copy()).cuda()
    units = fr.n_raw if fmt == WORDS else 2 * fr.n_raw
    out = torch.full((units * SIZE[fmt] + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    ver = torch.full((2,), 7, dtype=torch.int32, device="cuda")
    cfg = gpu.make_cfg(mode=1, **fr.kw); st = torch.cuda.current_stream().cuda_stream
    if fmt == RGB:
        gpu.decode_rgb_async(d.data_ptr(), d.numel() // 9, cfg, units, out.data_ptr(), ver.data_ptr(), st)
    else:
        assert gpu.decode_frame_async(d.data_ptr(), d.numel() // 9, cfg, fr.n_raw, out.data_ptr(), units, ver.data_ptr(), fmt == PIXELS, st) == units
    bounds.sync()
    return out[: units * SIZE[fmt]].cpu().numpy(), ver.cpu().tolist()


def outside(fr, far, fmt):
    """bool per output byte of a pixel format: the byte belongs to a pixel outside the pixel tiles of the refused blocks `far`"""
    keep = rp.pixels_outside_tiles(len(fr.padded), fr.ks[0], rp.far_tiles_one_k(fr.ks[0], far))
    return np.repeat(keep, SIZE[fmt])


def expected_pixels(orc, fr, exp, far):
    """The pixels the repaired stream `exp` of expected_erasures decodes to, by the oracle's decoder; the refused blocks `far` (as
    received in `exp`) are put back clean first, their tiles are not compared.  Outside those tiles this is fr.padded wherever every
    block was brought back to its own codeword -- a block beyond capacity may lie within reach of ANOTHER codeword, is accepted as that
    one by the rule, and then decodes to other pixels, which the yardstick's stream carries."""
    e = np.array(exp, np.uint8).reshape(-1); clean = fr.clean.reshape(-1)
    B = rp.block_index(fr.L, fr.ocfg); f0 = rp.band_first_block(fr.L)
    rows = np.array([f0[b] + m for b, m in far], np.int64)
    e[B[rows]] = clean[B[rows]]
    rc, px = orc.decode_frame(e.reshape(-1, 9), ol.make_cfg(mode=1))
    assert rc == 0 and len(px) == len(fr.padded)
    return px


def covers(orc, fr, s, kinds_of):
    """the damage plan's coverage per band, as test_gpu_erasures.test_erasure_sweep asserts it"""
    B = rp.block_index(fr.L, fr.ocfg); f0 = rp.band_first_block(fr.L)
    e_res = rp.field(orc).sub[s[B] % 27, fr.clean.reshape(-1)[B]]
    for b in range(9):
        rows = slice(f0[b], f0[b] + fr.blocks[b])
        hi = (s[B[rows]] > 26).sum(axis=1); er = ((e_res[rows] != 0) & (s[B[rows]] <= 26)).sum(axis=1)
        assert set(zip(hi.tolist(), er.tolist())) >= kinds_of(fr.ks[b]), (fr.name, b)


# ---- the recoverable sweep --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _recoverable(name, what):
    fr = _frame(name, what); orc = ol.oracle()
    only = ep.admissible(max(fr.ks)) + ["sched", "clean"]                    # admissible for every band: the pairs of the largest k
    s, _ = ep.damage_frame(orc, fr, SEED[what], only=only)
    _, words, far = ep.expected_erasures(orc, fr, s)
    assert words[1] == 0 and far == [] and words[4] == words[5] > 0 and (s > 26).any(), (name, what, words)
    s.setflags(write=False)
    return s, words[4]


@pytest.mark.parametrize("what", ("small", "padded"))
@pytest.mark.parametrize("name", sorted(rp.CONFIGS))
def test_recoverable_sweep(gpu, orc, name, what):
    """Every framing at two sizes, every admissible (s, e) in every band, nothing beyond capacity: the output is the frame's own pixels in
    every format its decoders produce, the words [0, 0, flagged, flagged]; the input is untouched at base offsets 0 and 2 mod 16, the
    output's guards intact under both fills."""
    fr = _frame(name, what)
    s, flagged = _recoverable(name, what)
    cfg = gpu.make_cfg(mode=1, **fr.kw)
    if what == "padded":
        covers(orc, fr, np.asarray(s), lambda k: set(ep.admissible(max(fr.ks))))
    for fmt in formats(name):
        assert gpu.decode_erasures_plan(fr.n_raw, cfg, fmt).path == (1 if name in FUSED and fmt != WORDS else 0), (name, fmt)
        want = want_bytes(orc, fr.padded, fmt)
        for offset, fill in ((0, bounds.FILLS[0]), (2, bounds.FILLS[1])):
            got, ver = run(gpu, fr, s, fmt, offset, fill)
            assert ver == [0, 0, flagged, flagged], (name, what, fmt, offset, ver, flagged)
            bounds.check_equal(got, want, fill, "decoded %s %s fmt %d at %d" % (name, what, fmt, offset))


# ---- beyond capacity ------------------------------------------------------------------------------------------------------------------------
EVERY_BEYOND = 29


@functools.lru_cache(maxsize=2)
def _beyond(name):
    fr = _frame(name, "padded"); orc = ol.oracle()
    s, planned = ep.damage_frame(orc, fr, 43, every=EVERY_BEYOND)
    exp, words, far = ep.expected_erasures(orc, fr, s)
    s.setflags(write=False)
    return s, words, far, expected_pixels(orc, fr, exp, far)


@pytest.mark.parametrize("name", FUSED)
def test_beyond_capacity(gpu, orc, name):
    """The full damage plan (every admissible pair, the beyond-capacity pairs, <= t rows, clean blocks): the words are the yardstick's,
    every pixel outside the tiles of the refused blocks is what the yardstick's stream decodes to (expected_pixels: the frame's own
    wherever no block was accepted as another codeword), and the synchronous entry returns T3_E_RS."""
    import torch
    fr = _frame(name, "padded")
    s, words, far, px = _beyond(name)
    same = px == fr.padded
    assert same[outside(fr, far, 1)[::6]].mean() > 0.5
    k = fr.ks[0]
    n_tiles = -(-max(fr.blocks) // 52)
    bad = rp.far_tiles_one_k(k, far)
    assert len(bad) >= n_tiles / 4 and n_tiles - len(bad) >= n_tiles / 4, (name, len(bad), n_tiles)       # checked before anything runs on the GPU
    covers(orc, fr, np.asarray(s), lambda kk: set(ep.admissible(kk)) | set(ep.beyond(kk)))
    assert 0 < words[5] < words[4] and words[1] >= words[4] - words[5], (name, words)
    want4 = [0, words[1], words[4], words[5]]
    for fmt in (PIXELS, RGB):
        assert gpu.decode_erasures_plan(fr.n_raw, gpu.make_cfg(mode=1, **fr.kw), fmt).path == 1
        got, ver = run(gpu, fr, s, fmt)
        assert ver == want4, (name, fmt, ver, want4)
        keep = outside(fr, far, fmt)
        assert keep.any() and np.array_equal(got[keep], want_bytes(orc, px, fmt)[keep]), (name, fmt)
    b = np.asarray(s)
    inb = bounds.Buf(len(b), FILL, 0, data=b, name="coded frame"); out = bounds.Buf(12 * fr.n_raw, FILL, 0, name="output")
    seen = gpu.DecoderContext(mode=1).cfg_last_seen
    rc, n, counts = gpu.decode_erasures_profile_dev(inb.ptr, len(b) // 9, seen, out.ptr, 2 * fr.n_raw, PIXELS, torch.cuda.current_stream().cuda_stream)
    bounds.sync()
    assert rc == gpu.E_RS and n == 2 * fr.n_raw and counts == want4, (name, rc, n, counts)
    inb.result()
    keep = outside(fr, far, PIXELS)
    assert np.array_equal(out.result()[keep], want_bytes(orc, px, PIXELS)[keep]), name


def test_beyond_capacity_generic(gpu, orc):
    """four_codes (path 0): the words alone."""
    fr = _frame("four_codes", "padded")
    s, words, far, _ = _beyond("four_codes")
    covers(orc, fr, np.asarray(s), lambda kk: set(ep.admissible(kk)) | set(ep.beyond(kk)))
    assert 0 < words[5] < words[4] and words[1] > 0
    for fmt in (PIXELS, WORDS):
        _, ver = run(gpu, fr, s, fmt)
        assert ver == [0, words[1], words[4], words[5]], (fmt, ver, words)


# ---- the contrast: what the mod-27 rule throws away ---------------------------------------------------------------------------------------
def test_flagged_bytes_are_decoded(gpu, orc):
    """The stream of test_gpu_erasures.test_flagged_bytes_are_recoverable: a k20 frame whose damaged blocks each hold 4..6 flagged bytes
    with wrong residues and no other error, left damaged only where the oracle's errors-only decoder refuses the residues.  The plain
    decoder reports failures; this entry returns the frame's pixels from the buffer as received, which it does not write."""
    fr = _frame("k20", "padded")
    F = rp.field(orc)
    s, planned = ep.damage_frame(orc, fr, 34, every=5, only=[(4, 0), (5, 0), (6, 0)], right=False, fill=False)
    clean = fr.clean.reshape(-1)
    B = rp.block_index(fr.L, fr.ocfg)
    s[int(B.max()) + 1:] = clean[int(B.max()) + 1:]
    e = F.sub[s[B] % 27, clean[B]]
    rows = np.flatnonzero((s[B] > 26).any(axis=1))
    _, _, ok = orc.rs_decode_blocks(20, e[rows], mode=1)
    s[B[rows[ok == 1]]] = clean[B[rows[ok == 1]]]                            # the errors-only rule accepts these residues: not part of the contrast
    rows = rows[ok != 1]
    hi = (s[B[rows]] > 26).sum(axis=1)
    assert len(rows) > 1000 and set(hi.tolist()) == {4, 5, 6} and not (s[B[rows]] % 27 == clean[B[rows]])[s[B[rows]] > 26].any()
    _, ver = plain(gpu, fr, s, PIXELS)
    assert ver[0] == 0 and ver[1] > 0, ver                                   # the decoder reports failures
    for fmt in (PIXELS, RGB, WORDS):                                        # path 1, path 1, path 0
        got, ver = run(gpu, fr, s, fmt)                                     # (run: the input buffer is unchanged)
        assert ver == [0, 0, len(rows), len(rows)], (fmt, ver, len(rows))
        bounds.check_equal(got, want_bytes(orc, fr.padded, fmt), FILL, "flagged bytes decoded, fmt %d" % fmt)


# ---- the rule's price -----------------------------------------------------------------------------------------------------------------------
def test_refused_blocks_are_not_retried_mod_27(gpu, orc):
    """A k24 frame (r = 2) with blocks of one flagged byte plus one error elsewhere: 2 * 1 + 1 > 2, refused.  Where the flagged byte's
    residue happens to be right the errors-only decoder accepts the block -- the plain decoder run on path 0's repaired copy does --, and
    word [1] counts it all the same, equally on both paths."""
    fr = _frame("k24", "padded")
    F = rp.field(orc)
    s, _ = ep.damage_frame(orc, fr, 44, every=7, only=[(1, 1)], fill=False)
    _, words, far = ep.expected_erasures(orc, fr, s)
    clean = fr.clean.reshape(-1); B = rp.block_index(fr.L, fr.ocfg); f0 = rp.band_first_block(fr.L)
    rows = np.array([f0[b] + m for b, m in far])
    assert words[1] == len(rows) > 1000 and words[4] >= words[1] and (s[B[rows]] > 26).sum(axis=1).tolist() == [1] * len(rows)
    _, _, ok = orc.rs_decode_blocks(24, F.sub[s[B[rows]] % 27, clean[B[rows]]], mode=1)
    assert 0 < int((ok == 1).sum()) < len(rows)                              # the mod-27 rule would accept some of the refused blocks
    want4 = [0, words[1], words[4], words[5]]
    cfg = gpu.make_cfg(mode=1, **fr.kw)
    for fmt, path in ((PIXELS, 1), (WORDS, 0)):                              # path 0 is forced by asking for raw words
        assert gpu.decode_erasures_plan(fr.n_raw, cfg, fmt).path == path
        _, ver = run(gpu, fr, s, fmt)
        assert ver == want4, (fmt, ver, want4)
    _, pv = plain(gpu, fr, s, PIXELS)
    assert pv[1] < words[1], (pv, words)                                     # the plain decoder under-reports


# ---- no byte above 26: the plain decoders -------------------------------------------------------------------------------------------------
def check_plain_cases(gpu, orc, name, what, cases):
    fr = _frame(name, what)
    for case in cases:
        stream, M, where = fr.stream(case)
        assert not (np.asarray(stream) > 26).any()
        for fmt in formats(name):
            want, w2 = plain(gpu, fr, stream, fmt)
            got, w4 = run(gpu, fr, stream, fmt)
            assert w4 == w2 + [0, 0] and w2 == [0, M], (name, what, case, fmt, w4, w2)
            if M == 0:
                assert np.array_equal(got, want), (name, what, case, fmt)
            elif fmt != WORDS and name in rp.ONE_K and what != "small":      # tiles are independent: the rest of the frame still decodes
                keep = outside(fr, where, fmt)
                assert keep.any() and np.array_equal(got[keep], want_bytes(orc, fr.padded, fmt)[keep]), (name, what, case, fmt)


@pytest.mark.parametrize("what", ("small", "padded"))
@pytest.mark.parametrize("name", sorted(rp.CONFIGS))
def test_without_flagged_bytes_is_the_plain_decoder(gpu, orc, name, what):
    """On the streams of rs_patterns.CASES (no byte above 26): bytes and words [0], [1] of t3hip_decode_frame_async / _rgb_async,
    [2] = [3] = 0; with far rows the words, and the pixels outside the far tiles."""
    check_plain_cases(gpu, orc, name, what, rp.CASES[what])


@pytest.mark.parametrize("name", ("k20", "uep_18_22"))
def test_near_rows_decode_as_the_plain_decoder(gpu, orc, name):
    """'near' (blocks beyond t within t of another codeword: accepted, decoded to that codeword) exists at the full size only."""
    check_plain_cases(gpu, orc, name, "full", ("near",))


# ---- the tile loop ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,per_cu", (("k20", 9), ("k20_beacon83", 3)))
def test_tile_loop(gpu, orc, name, per_cu):
    """One k20 frame of per_cu x CU count + 1 tiles, ragged last tile, as test_gpu_erasures.test_tile_loop builds its own: every workgroup
    (two per CU) walks its loop more than twice, with tagged entries in every pass; the damage plan thinned to every 701st block."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    tiles = per_cu * cus + 1
    n_px = tiles * 108 * 20 - 1001                                          # the last tile ragged, the count odd
    cfg = gpu.make_cfg(mode=1, **rp.CONFIGS[name])
    fr = rp.Frame(orc, lambda n_raw: gpu.plan(n_raw, cfg), name, n_px, 103)
    p = gpu.decode_erasures_plan(fr.n_raw, cfg, PIXELS)
    assert p.path == 1 and p.n_tiles == tiles
    every = 701 if per_cu == 9 else 233
    s, planned = ep.damage_frame(orc, fr, 33, every=every)
    exp, words, far = ep.expected_erasures(orc, fr, s)
    px = expected_pixels(orc, fr, exp, far)
    f0 = rp.band_first_block(fr.L)
    at = np.concatenate([np.flatnonzero(planned[f0[b]: f0[b] + fr.blocks[b]]) // 52 for b in range(9)])     # the tiles that hold a planned block
    passes = range(0, tiles - 1, 2 * cus)
    assert len(passes) > 2 or per_cu < 4
    assert all(((at >= lo) & (at < min(lo + 2 * cus, tiles))).sum() > 30 for lo in passes) and words[5] > 300   # in every pass of the loop
    got, ver = run(gpu, fr, s, PIXELS)
    assert ver == [0, words[1], words[4], words[5]], (ver, words)
    keep = outside(fr, far, PIXELS)
    assert keep.sum() > len(keep) // 2 and np.array_equal(got[keep], want_bytes(orc, px, PIXELS)[keep])
    assert (px == fr.padded)[keep[::6]].mean() > 0.9                        # (a block accepted as another codeword is rare here)


# ---- the synchronous entries ------------------------------------------------------------------------------------------------------------
def _damage_header(stream, n):
    """n symbol errors in the header's first RS(26,18) block (t = 4)"""
    s = np.ascontiguousarray(stream, np.uint8).copy().reshape(-1)
    at = np.arange(n) * 2 + 1
    s[at] = (s[at] + 1 + np.arange(n) % 25) % 27
    return s


@pytest.mark.parametrize("name", ("k20", "four_codes"))
def test_profile_entries(gpu, orc, name):
    """One fused and one generic configuration: a damaged but decodable header decodes (counts[0] stays 0), `seen` is the frame's
    configuration; a header damaged beyond t is T3_E_HEADER with nothing written to the output."""
    import torch
    fr = _frame(name, "small")
    ok_s, flagged = _recoverable(name, "small")
    mixed = ep.damage_frame(orc, fr, 45)[0]
    _, mw, _ = ep.expected_erasures(orc, fr, mixed)
    assert mw[1] > 0
    st = torch.cuda.current_stream().cuda_stream
    want_cfg = gpu.make_cfg(mode=1, **fr.kw)
    cases = (("clean header", np.asarray(ok_s), gpu.OK, [0, 0, flagged, flagged]), ("header+2", _damage_header(ok_s, 2), gpu.OK, [0, 0, flagged, flagged]),
             ("mixed", mixed, gpu.E_RS, [0, mw[1], mw[4], mw[5]]), ("header+9", _damage_header(ok_s, 9), gpu.E_HEADER, [0, 0, 0, 0]))
    for label, s, want_rc, want4 in cases:
        for fmt in formats(name):
            tag = (name, label, fmt)
            units = fr.n_raw if fmt == WORDS else 2 * fr.n_raw
            inb = bounds.Buf(len(s), FILL, 2, data=s, name="coded frame"); out = bounds.Buf(units * SIZE[fmt], FILL, 0, name="output")
            seen = gpu.DecoderContext(mode=1).cfg_last_seen
            rc, n, counts = gpu.decode_erasures_profile_dev(inb.ptr, len(s) // 9, seen, out.ptr, units, fmt, st)
            bounds.sync()
            assert rc == want_rc and counts == want4, (tag, rc, counts, want4)
            inb.result()
            if want_rc == gpu.E_HEADER:
                assert n == 0
                out.untouched()
            else:
                assert n == units and seen.profile == want_cfg.profile and list(seen.band_profile) == list(want_cfg.band_profile) and seen.mode == 1, tag
                if want_rc == gpu.OK:
                    out.expect(want_bytes(orc, fr.padded, fmt))
            before = s.copy()
            rc, got, counts = gpu.decode_erasures_profile(s.reshape(-1, 9), gpu.DecoderContext(mode=1), fmt)
            assert rc == want_rc and counts == want4 and np.array_equal(s, before), (tag, "host", rc, counts)
            if want_rc == gpu.E_HEADER:
                assert got.size == 0, tag
            elif want_rc == gpu.OK:
                assert np.array_equal(np.ascontiguousarray(got).view(np.uint8).reshape(-1), want_bytes(orc, fr.padded, fmt)), (tag, "host")
    with pytest.raises(gpu.T3Error) as e:                                     # seen->mode must be FIXED on entry
        gpu.decode_erasures_profile(np.asarray(ok_s).reshape(-1, 9), gpu.DecoderContext(mode=0), PIXELS)
    assert e.value.code == gpu.E_ARG
