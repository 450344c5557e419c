"""The four in-place repairs -- repair_fixed_kernel<R> / repair_generic_kernel, repair_frames_kernel<R>, erasure_fixed_kernel<R> /
erasure_generic_kernel, erasure_frames_kernel<R> -- at every place a frame can end within their tiles, with a dirty tail.

The sizes are tests/repair_ends.py's lattice (every word count up to 130, both sides of every tile boundary up to one fused tile plus
two block rows, the first three steps of each launch's tile count); the streams are its end_damage: the last block of every band
carries an (erased, wrong) kind, every tail byte is dirty -- canonical values 1..26 among them, which only a store of the tail can
remove --, every beacon slot holds a seeded byte, every 7th frame ends in a refused block.  tests/test_repair_ends_lattice.py proves on
the CPU that the lattice holds the plans' steps and that the streams reach those places.

The yardsticks are test_repair_semantics.expected (the oracle's block decoder) and erasure_patterns.expected_erasures, computed once per
configuration.  Every buffer is tests/bounds.py's: the frame's bytes between guards, at base offsets 0, 2, .. 14 behind a 16-byte
boundary and with both fills in turn.  These kernels store next to bytes that must not change -- a refused block, the gap of a stride,
the next frame's header, bytes behind the frame's own words --, so every comparison is exact and covers every byte."""
import numpy as np
import pytest

import bounds
import oracle_lib as ol
import repair_ends as re
import rs_patterns as rp
from test_gpu_erasure_frames import run_batch                              # (checks the GAP bytes of a stride and the SPARE words itself)
from test_gpu_erasures import run
from test_repair_semantics import FUSED, SWEEP

pytestmark = pytest.mark.gpu
BATCHED = FUSED + ("k20_beacon83", "four_codes")  # one launch; the loop of the single-frame body with a beacon and with four codes
STRIDE_EXTRA = 4112
POOL = 7                                          # distinct frames cycled over a batch of one-tile frames


def want(c, era):
    """(R', verdict words) of a case: the erasure yardstick's six words, or [0] + the plain yardstick's three"""
    return (c.era, c.era_words) if era else (c.plain, [0] + c.plain_words)


def second(words, era):
    """The words of a repair of R': refused blocks are refused again, nothing changes"""
    return [0, words[1], 0, 0, words[4] - words[5], 0] if era else [0, words[1], 0, 0]


def run_wide(gpu, fr, stream, extra, offset, fill, era):
    """One repair call that is told of `extra` words more than the frame holds, those bytes holding the fill -> (the frame's bytes
    afterwards, the verdict words); bounds.Buf checks that the bytes behind the frame's own words stay."""
    import torch
    b = np.ascontiguousarray(stream, np.uint8).reshape(-1)
    data = np.concatenate([b, np.full(9 * extra, fill, np.uint8)])
    buf = bounds.Buf(len(data), fill, offset, data=data, name="frame and %d words" % extra, may_change=((0, len(b)),))
    ver = torch.full((8,), 7, dtype=torch.int32, device="cuda")
    fn = gpu.repair_erasures_frame_async if era else gpu.repair_frame_async
    fn(buf.ptr, len(data) // 9, gpu.make_cfg(mode=1, **fr.kw), fr.n_raw, gpu.REPAIR_WRITE, ver.data_ptr(), torch.cuda.current_stream().cuda_stream)
    bounds.sync()
    v = ver.cpu().tolist()
    nw = 6 if era else 4
    assert v[nw:] == [7] * (8 - nw), "words behind the verdict were written"
    return buf.result()[: len(b)], v[:nw]


def sweep_of(name, salt, era):
    """The cases of a sweep; the plain repair's tests do not wait for the erasure yardstick"""
    return re.cases(name, salt) if era else re.plain_cases(name, salt)


def sweep_single(gpu, name, era):
    for c in sweep_of(name, 0, era):
        fr, i = c.fr, c.i
        exp, words = want(c, era)
        offset, fill = 2 * (i % 8), bounds.FILLS[i % 2]
        tag = (name, "erasures" if era else "plain", c.W, fr.n_px)
        got, ver = run(gpu, fr, c.rec, gpu.REPAIR_WRITE, offset, fill, era=era)
        assert ver == words, (tag, "words", ver, words)
        bounds.check_equal(got, exp, fill, "repaired %s" % (tag,))
        if i % 5 == 0:                                                       # a dry run: the same words, no byte stored
            got, ver = run(gpu, fr, c.rec, 0, offset, fill, era=era)
            assert ver == words, (tag, "dry run", ver, words)
            assert np.array_equal(got, c.rec), (tag, "dry run wrote")
        if i % 5 == 2:                                                       # R' again: nothing left to change
            got, ver = run(gpu, fr, exp, gpu.REPAIR_WRITE, offset, fill, era=era)
            assert ver == second(words, era), (tag, "second repair", ver, words)
            assert np.array_equal(got, exp), (tag, "second repair wrote")
        if i % 10 == 4:                                                      # n_in above the plan's words: the bytes behind them stay
            for extra in (1, 2):
                got, ver = run_wide(gpu, fr, c.rec, extra, offset, fill, era)
                assert ver == words, (tag, "n_in + %d" % extra, ver, words)
                bounds.check_equal(got, exp, fill, "repaired %s with n_in + %d" % (tag, extra))


@pytest.mark.parametrize("name", SWEEP)
def test_repair_at_every_frame_end(gpu, orc, name):
    """t3hip_repair_frame_async on every lattice frame: the buffer is the yardstick's R', the words are its words, the guards and the
    words behind the verdict are untouched; every 5th frame also as a dry run, every 5th a second time, every 10th with n_in one and
    two words above the frame's."""
    sweep_single(gpu, name, False)


@pytest.mark.parametrize("name", SWEEP)
def test_erasure_repair_at_every_frame_end(gpu, orc, name):
    """t3hip_repair_erasures_frame_async on the same streams against the erasure yardstick's bytes and six words."""
    sweep_single(gpu, name, True)


# ---- batches ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,era", [(n, e) for n in BATCHED for e in (False, True)])
def test_batched_repairs_at_every_frame_end(gpu, orc, name, era):
    """t3hip_repair_frames_async / t3hip_repair_erasures_frames_async, three different frames per lattice size (content and damage of
    salts 0, 1, 2; frames 0 and 1 of every 7th size end in a refused block), strides minimal and + 4112 with the gaps filled in turn:
    in the tile space frame f's last tile, and its tail, are followed by frame f + 1's header and first tile.  Every frame's bytes and
    words are the single-frame yardstick's; test_gpu_erasure_frames.run_batch looks at every gap byte, the guards and the spare words."""
    sweeps = [sweep_of(name, salt, era) for salt in (0, 1, 2)]
    cfg = gpu.make_cfg(mode=1, **rp.CONFIGS[name])
    for i, W in enumerate(re.repair_lattice(name)):
        cs = [s[i] for s in sweeps]
        fr = cs[0].fr
        assert all(c.fr.n_raw == W and c.fr.n_px == fr.n_px for c in cs) and len({c.rec.tobytes() for c in cs}) == 3, (name, W)
        p = gpu.repair_frames_plan(W, 3, cfg)
        assert p.one_launch == p.path == (1 if name in FUSED else 0), (name, W)
        stride = p.stride_min + (STRIDE_EXTRA if i % 2 else 0)
        got, ver = run_batch(gpu, fr, [c.rec for c in cs], gpu.REPAIR_WRITE, stride=stride, offset=2 * (i % 8), fill=bounds.FILLS[i % 2], era=era)
        hs = int(fr.L.header_syms)
        for f, c in enumerate(cs):
            exp, words = want(c, era)
            tag = (name, "erasures" if era else "plain", W, stride, "frame %d" % f)
            assert ver[f] == words, (tag, "words", ver[f], words)
            bounds.check_equal(got[f], exp, bounds.FILLS[i % 2], "repaired %s" % (tag,))
            assert np.array_equal(got[f][:hs], c.rec[:hs]), (tag, "header")


def one_tile_pool(gpu, orc):
    """POOL k20 frames of one size from the dense run -- one fused tile, an odd pixel count, the longest tail there is among them --,
    different in content and damage, frame 3 ending in a refused block"""
    cfg = gpu.make_cfg(mode=1, **rp.CONFIGS["k20"])
    ocfg = ol.make_cfg(mode=1, **rp.CONFIGS["k20"])
    dense = [(len(re.tail_parts(gpu.plan(W, cfg), ocfg)[0]), W, i) for i, W in enumerate(re.repair_lattice("k20")) if 20 <= W <= 130 and i % 2 == 1]
    tail, W, i = max(dense)
    assert tail >= 1
    return [re.make_case(orc, "k20", W, i + 2 * j, salt=10 + j, far=j == 3) for j in range(POOL)]   # (i picks the kinds; + 2 j keeps the pad pixel)


@pytest.mark.parametrize("era", (False, True))
def test_many_one_tile_frames(gpu, orc, era):
    """More one-tile frames than the launch has workgroups: 9 x CU count + 1 frames at the smallest even stride, so that every workgroup
    of the persistent grid (at most three a CU) strides over more than two frames, each with a tail to store and counts to flush."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n_frames = 9 * cus + 1
    pool = one_tile_pool(gpu, orc)
    fr = pool[0].fr
    assert fr.n_px % 2 == 1 and len({c.rec.tobytes() for c in pool}) == POOL and [c.far for c in pool].count(True) == 1
    assert n_frames < 65535 and len({tuple(want(c, era)[1]) for c in pool}) >= POOL - 2     # words that tell a frame from its neighbours
    p = gpu.repair_frames_plan(fr.n_raw, n_frames, gpu.make_cfg(mode=1, **fr.kw))
    assert p.tiles_per_frame == 1 and p.one_launch == 1 and p.stride_min % 2 == 0
    cs = [pool[f % POOL] for f in range(n_frames)]
    got, ver = run_batch(gpu, fr, [c.rec for c in cs], gpu.REPAIR_WRITE, stride=p.stride_min, era=era)
    for f, c in enumerate(cs):
        exp, words = want(c, era)
        assert ver[f] == words, ("one-tile frames", era, f, ver[f], words)
        bounds.check_equal(got[f], exp, bounds.FILLS[0], "one-tile frame %d of %d" % (f, n_frames))


# ---- the synchronous entries ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("era", (False, True))
def test_profile_entries_at_frame_ends(gpu, orc, era):
    """t3hip_repair_profile_dev / t3hip_repair_profile (with era: the _erasures_ entries) on every 10th lattice frame of a fused and a
    beaconed framing; the frame's size comes from its header, which is clean: counts[0] = 0, T3_E_RS exactly where a block is refused."""
    import torch
    dev, host = (gpu.repair_erasures_profile_dev, gpu.repair_erasures_profile) if era else (gpu.repair_profile_dev, gpu.repair_profile)
    refused = 0
    for name in ("k20", "k22_beacon2_slot8"):
        for c in sweep_of(name, 0, era)[::10]:
            exp, words = want(c, era)
            want_rc = gpu.E_RS if words[1] else gpu.OK
            refused += 1 if words[1] else 0
            assert not c.far or want_rc == gpu.E_RS
            tag = (name, era, c.W)
            fill = bounds.FILLS[c.i // 10 % 2]
            buf = bounds.Buf(len(c.rec), fill, 0, data=c.rec, name="frame", may_change=((0, len(c.rec)),))
            rc, counts = dev(buf.ptr, len(c.rec) // 9, gpu.DecoderContext(mode=1).cfg_last_seen, gpu.REPAIR_WRITE, torch.cuda.current_stream().cuda_stream)
            bounds.sync()
            assert rc == want_rc and counts == words and counts[0] == 0, (tag, rc, counts, words)
            bounds.check_equal(buf.result(), exp, fill, "profile_dev %s" % (tag,))
            w = c.rec.copy().reshape(-1, 9)
            rc, counts = host(w, gpu.DecoderContext(mode=1), gpu.REPAIR_WRITE)
            assert rc == want_rc and counts == words, (tag, "host", rc, counts, words)
            assert np.array_equal(w.reshape(-1), exp), (tag, "host")
    assert refused > 0
