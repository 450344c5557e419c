"""The frames of tests/wild_inputs.py are what tests/test_gpu_wild_inputs.py takes them for: proven here with the CPU oracle alone.

Every (pixel, component) and every (word, byte) is wild exactly once over the full sweeps and never closer than P to the next wild value of
its frame, and every listed value meets every component and byte slot of a lane's work unit; the base frames are in range and span the tile boundaries claimed (tests/golden/enc_plan.json, the library's host-only batch
plan); every listed value lies outside the range, next to the edge it is listed for.  And the planted failures: for every frame of the full
sweeps the oracle's stream changes when the frame's wild values are clamped to the range instead, or lose their upper byte -- a converter
that missed the reduction in one of these ways could not produce the expected stream of any frame."""
import json
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as ol
import wild_inputs as wi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K20 = dict(profile=2, uep=2)


def n_sym(W):
    return -(-26 * W // 3)


# ---- the sweeps ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [wi.W_BASE, wi.W_BIG])
def test_every_pixel_component_is_wild_once(W):
    n = wi.n_px_of(W)
    hits = np.zeros((n, 3), np.int64)
    met = set()                                                               # (pixel slot of the lane unit, component, value)
    for c in wi.PIXEL_SWEEPS:
        for s in range(wi.P):
            at, comp, cyc = wi.pixel_sites(n, c, s)
            assert len(at) >= 1 and at[0] == s and (np.diff(at) == wi.P).all(), (c, s)
            np.add.at(hits, (at, comp), 1)
            vals = [wi.wild_pixel_value(int(k), int(q)) for k, q in zip(comp, cyc)]
            assert len(set(vals)) >= 4, (c, s, vals)                          # a frame's values differ
            met.update((int(a) % wi.LANE_UNIT, int(k), v) for a, k, v in zip(at, comp, vals))
    assert (hits == 1).all()
    # every listed value in each of the 12 x 3 component slots of a lane unit: low and high half of both register pairs
    assert met == {(slot, k, v) for slot in range(wi.LANE_UNIT) for k in range(3) for v in (wi.Y_WILD if k == 0 else wi.C_WILD)}
    per_sweep = np.zeros(n, np.int64)                                         # the thinned sweep: every pixel once, the components cycling
    comps = set()
    for s in range(wi.P):
        at, comp, _ = wi.pixel_sites(n, 0, s)
        per_sweep[at] += 1; comps.update(int(k) for k in comp)
    assert (per_sweep == 1).all() and comps == {0, 1, 2}


@pytest.mark.parametrize("W", [wi.W_BASE, wi.W_BIG])
def test_every_word_byte_is_wild_once(W):
    hits = np.zeros((W, 9), np.int64)
    first3 = np.zeros((12, 9), np.int64)                                      # (word within its lane unit of twelve, byte) over sweeps 0, 1, 2
    met = set()                                                               # (word slot of the lane unit, byte, value)
    for c in wi.WORD_SWEEPS:
        for s in range(wi.P):
            at, b, cyc = wi.word_sites(W, c, s)
            assert len(at) >= 1 and at[0] == s and (np.diff(at) == wi.P).all(), (c, s)
            np.add.at(hits, (at, b), 1)
            if c < 3:
                np.add.at(first3, (at % 12, b), 1)
            vals = [wi.wild_byte_value(int(q)) for q in cyc]
            assert len(set(vals)) >= 3, (c, s, vals)
            met.update((int(a) % wi.LANE_UNIT, int(k), v) for a, k, v in zip(at, b, vals))
        assert (hits.sum(axis=1) == c + 1).all()                              # every sweep on its own: every word once
    assert (hits == 1).all()
    assert (first3 > 0).all()
    assert met == {(slot, k, v) for slot in range(wi.LANE_UNIT) for k in range(9) for v in wi.B_WILD}   # every value in each of the 12 x 9 byte slots


def test_frames_are_the_base_frame_but_for_their_wild_values():
    """The frames as built (sweep 1 of each front end, both base sizes for pixels): they differ from the base exactly at the listed sites, by the
    listed values; the base is in range, with trit 26 set in many words."""
    for W in (wi.W_BASE, wi.W_BIG):
        base = wi.base_pixels(W)
        assert len(base) % 2 == 1 and base["Yq"].max() == 242 and base["Yq"].min() == 0
        for k in ("Cbq", "Crq"):
            assert base[k].min() == -40 and base[k].max() == 40
        for s in (0, 1, 400, wi.P - 1):
            px = wi.pixel_frame(W, 1, s)
            at, comp, cyc = wi.pixel_sites(len(px), 1, s)
            diff = np.zeros((len(px), 3), bool)
            for i, k in enumerate(wi.COMPONENTS):
                diff[:, i] = px[k] != base[k]
            want = np.zeros_like(diff); want[at, comp] = True
            assert np.array_equal(diff, want), (W, s)
            for a, k, q in zip(at, comp, cyc):
                assert int(px[wi.COMPONENTS[k]][a]) == wi.wild_pixel_value(int(k), int(q))
    raw0 = wi.base_words(wi.W_BASE)
    assert raw0.max() == 26 and (raw0[:, 8] >= 18).mean() > 0.25              # (byte 8 >= 18: trit 26 is 2, >= 9: it is set)
    for s in (0, 1, 400, wi.P - 1):
        raw = wi.word_frame(wi.W_BASE, 1, s)
        at, b, cyc = wi.word_sites(wi.W_BASE, 1, s)
        want = np.zeros(raw.shape, bool); want[at, b] = True
        assert np.array_equal(raw != raw0, want), s
        assert [int(raw[a, k]) for a, k in zip(at, b)] == [wi.wild_byte_value(int(q)) for q in cyc]


def test_listed_values_lie_next_to_their_edges():
    """What the reference makes of each listed value (the uint32 cast mod 3^w, a byte mod 27), and the edge it stands at."""
    red_y = lambda v: v % 243
    red_c = lambda v: ((v + 40) % (1 << 32)) % 81
    assert [red_y(v) for v in wi.Y_WILD] == [0, 1, 242, 0, 206, 168]           # 243 | 244: first values out of range; 485 | 486: the second wrap;
    assert all(242 < v < 65536 for v in wi.Y_WILD) and max(wi.Y_WILD) == 65535  # 32768: the sign bit of a 16-bit half; 65535: the largest
    assert [red_c(v) for v in wi.C_WILD] == [0, 1, 48, 47, 80, 0, 2, 45]       # 41 | 42 above; -41 | -42 below: the cast wraps (2^32 = 49 mod 81);
    assert all(not -40 <= v <= 40 and -32768 <= v <= 32767 for v in wi.C_WILD)  # 121 | 122: C + 40 = 161 | 162, the second wrap; the int16 extremes
    assert [v % 27 for v in wi.B_WILD] == [0, 19, 20, 19, 20, 12] and all(26 < v < 256 for v in wi.B_WILD)
    bit7 = lambda b: ((b | (b + 0x65)) & 0x80) != 0                            # the word converter's test, one byte of it (a carry leaves the byte)
    plus = lambda b: ((b + 0x65) & 0x80) != 0
    assert not bit7(26) and plus(27) and plus(127) and not 127 & 0x80          # 27: the first; 127 | 128: bit 7 of the byte itself;
    assert 128 & 0x80 and plus(154) and not plus(155) and 155 & 0x80           # 154 | 155: b + 0x65 = 255 | 256, the sum's bit 7 goes with the carry
    assert all(bit7(b) == (b > 26) for b in range(256))


# ---- base sizes ----------------------------------------------------------------------------------------------------------------------------
def test_base_frames_span_the_recorded_tiles(t3):
    with open(os.path.join(ROOT, "tests", "golden", "enc_plan.json")) as f:
        found = [g for g in json.load(f) if g["found"]]
    tiles = {(g["kind"], g["block"], 9 * g["Lq"]) for g in found}
    assert max(t for k, _, t in tiles if k in ("MfmaK", "Uep")) == 12096 and max(t for _, _, t in tiles) == 29808
    assert (("Lut", 704, 14256) in tiles) and (("Lut", 1024, 29808) in tiles)
    small, big = n_sym(wi.W_BASE), n_sym(wi.W_BIG)
    assert (small, big) == (30342, 59809)
    for kind, block, tile in tiles:
        assert small > tile and big > 2 * tile and big % tile, (kind, block, tile)                  # one boundary inside / two and a ragged end
        if tile <= 14256:
            assert small > 2 * tile and small % tile, (kind, block, tile)
    for mode in (0, 1):                                                          # the library's own count for the full sweeps' pixel frames
        p = t3.frames_plan(False, wi.n_px_of(wi.W_BASE), 3 * wi.P, t3.make_cfg(mode=mode, **K20), t3.FRAMES_PIXELS)
        assert p.one_launch == 1 and p.tiles_per_frame >= 3, (mode, p.tiles_per_frame)
        assert p.in_bytes == 6 * wi.n_px_of(wi.W_BASE)


@pytest.fixture(scope="module")
def dispatch(tmp_path_factory):
    """tests/cpp/enc_dispatch_demo.cpp on every thinned configuration and the full sweeps', both front ends -> {(name, front end): launches}"""
    csrc = os.path.join(ROOT, "ternary-image-codec_amd", "csrc")
    exe = str(tmp_path_factory.mktemp("enc_dispatch") / "enc_dispatch_demo")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wno-unknown-pragmas", "-I" + csrc, os.path.join(ROOT, "tests", "cpp", "enc_dispatch_demo.cpp"),
                    os.path.join(csrc, "t3_enc_plan.cpp"), os.path.join(csrc, "t3_host.cpp"), "-o", exe], check=True)
    cases = dict(wi.THINNED, k20_fixed=(K20, 1, wi.W_BASE, [("MfmaK", 512, 0, 0)], [("MfmaK", 512, 0, 0)]))
    keys, args = [], []
    for name, (kw, mode, W, _, _) in cases.items():
        c = ol.make_cfg(mode=mode, **kw)
        for fe, front_end in enumerate(("pixels", "words")):
            keys.append((name, front_end))
            args += [c.profile, *c.band_profile, c.tile_w, c.tile_h, mode, fe, W]
    out = json.loads(subprocess.run([exe] + [str(a) for a in args], check=True, capture_output=True, text=True).stdout)
    return cases, dict(zip(keys, out))


def test_configurations_take_the_paths_named_for_them(dispatch):
    """The kernel kind, workgroup size and 2-D flow of every launch, as plan_encode's grouping and the tile planner give them; every launch
    has two tile boundaries and a ragged last tile inside the configuration's base frame."""
    cases, launches = dispatch
    for name, (kw, mode, W, px, words) in cases.items():
        for front_end, want in (("pixels", px), ("words", words)):
            got = launches[(name, front_end)]
            assert [(g["kind"], g["block"], g["il_on"], g["il_async"]) for g in got] == want, (name, front_end, got)
            for g in got:
                assert g["n_tiles"] >= 3 and n_sym(W) > 2 * g["tile"] and n_sym(W) % g["tile"], (name, front_end, g)
    # what the store flows of convert_pixels_packed and the passes behind it branch on (t3_encode.h)
    assert launches[("2d_513x8_k20", "pixels")][0]["il_w"] % 4 != 0                # IL = 2, not rows4: symbol-by-symbol stores
    assert launches[("2d_1024x16_k20", "pixels")][0]["il_w"] % 4 == 0              # IL = 2, rows4: the run-placed flow
    assert launches[("2d_64x64_luma", "pixels")][0]["il_w"] % 16 == 0 and launches[("2d_512x8_three_codes", "pixels")][0]["il_w"] % 16 == 0   # IL = 1: reverse_rows16
    assert launches[("2d_7x5_k22", "pixels")][0]["il_w"] % 4 != 0                  # IL = 1: permute_rows, symbol by symbol
    assert len(launches[("four_codes", "pixels")]) == 2 and len(launches[("four_codes", "words")]) == 2


# ---- planted failures ------------------------------------------------------------------------------------------------------------------------
def differs_everywhere(front_end, c, change):
    sw = wi.sweep(front_end, K20, 1, cs=(c,))
    make = wi.pixel_frame if front_end == "pixels" else wi.word_frame
    got = wi.pool(lambda s: wi.encode(front_end, make(wi.W_BASE, c, s, change), sw.ocfg), range(wi.P))
    same = [s for s in range(wi.P) if np.array_equal(got[s], sw.want[s])]
    assert not same, (front_end, c, change.__name__, same[:10])


@pytest.mark.parametrize("change", [wi.clamp_pixel, wi.low_byte_pixel], ids=["clamped", "low_byte"])
@pytest.mark.parametrize("c", wi.PIXEL_SWEEPS)
def test_planted_failures_change_every_pixel_frame(orc, c, change):
    """RS(26,20), FIXED: the stream of every frame of the sweep differs from the expected one when its wild values are (a) clamped to the
    nearest in-range value, (b) taken mod 256.  (Single values can survive one of the two -- 485 clamps to 242 = 485 % 243, 243 mod 256 is
    243 -- but no value survives both except chroma 121, whose frames hold other values too.)"""
    differs_everywhere("pixels", c, change)


@pytest.mark.parametrize("c", wi.WORD_SWEEPS)
def test_planted_failures_change_every_word_frame(orc, c):
    """... when its wild bytes are saturated at 26, the nearest in-range value (no listed value is 26 mod 27, nor 8 mod 9 where only two
    trits of the byte reach the stream)."""
    assert all(v % 27 != 26 and (v % 27) % 9 != 8 for v in wi.B_WILD)
    differs_everywhere("words", c, wi.clamp_byte)


def test_a_single_wild_value_changes_the_stream(orc):
    """Value by value, at one site: the oracle's stream with the value differs from the stream with it clamped or with its low byte, in one of
    the two at least (chroma 121 excepted: 161 % 81 = 80 is what 40 gives as well)."""
    ocfg = ol.make_cfg(mode=1, **K20)
    base = wi.base_pixels(wi.W_BASE)
    for comp, values in ((0, wi.Y_WILD), (1, wi.C_WILD), (2, wi.C_WILD)):
        for v in values:
            out = []
            for change in (None, wi.clamp_pixel, wi.low_byte_pixel):
                px = base.copy()
                w = v if change is None else change(comp, v)
                px[wi.COMPONENTS[comp]][1000] = w & 0xFFFF if comp == 0 else np.array(w).astype(np.int16)
                out.append(wi.encode("pixels", px, ocfg))
            survives = [np.array_equal(out[0], o) for o in out[1:]]
            assert survives == [True, True] if v == 121 else not all(survives), (comp, v, survives)


# ---- exhaustive frames ---------------------------------------------------------------------------------------------------------------------
def test_exhaustive_pixels_hold_every_value_in_every_slot(orc):
    px = wi.exhaustive_pixels()
    assert len(px) % 2 == 1
    slot = np.arange(len(px)) % 3
    for i, k in enumerate(wi.COMPONENTS):
        seen = np.zeros((3, 65536), bool)
        seen[slot, px[k].astype(np.int64) & 0xFFFF] = True
        assert seen.all(), k
    comps = wi.reduced_components(px)
    assert comps[:, 0].max() == 242 and comps[:, 1:].max() == 80 and comps.min() == 0
    assert np.array_equal(orc.pack_pixels(px), wi.words_of_components(comps)), "the oracle's packer against Y % 243 and ((C + 40) mod 2^32) % 81"


def test_exhaustive_words_hold_every_byte_in_every_slot(orc):
    raw = wi.exhaustive_words()
    assert len(raw) % 2 == 1 and (raw.reshape(-1) > 26).mean() > 0.85
    unit = raw[:3072].reshape(256, 108)                                       # lane units of four word triples
    for p in range(108):
        assert len(set(unit[:, p].tolist())) == 256, p
    assert np.array_equal(orc.regroup(raw), orc.regroup(raw % 27)), "the reference reduces every byte mod 27"
