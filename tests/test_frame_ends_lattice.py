"""The lattice of tests/frame_ends.py holds both sides of every tile step: proven here without a GPU and without taking a size from the
code under test.  The lattice is built from the band codes alone; the library's host-only plans (t3hip_frames_plan, t3hip_window_plan)
and the recorded encoder plans (tests/golden/enc_plan.json, tied to the planner by test_enc_plan.py) say where the tile count of each
kernel really steps, and every such place must be in it."""
import json
import os

import pytest

import frame_ends as fe
import rs_patterns as rp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W_MAX = fe.w_le(fe.CAP) + 1
ENCODER_CONFIGS = dict(rp.CONFIGS, **{"2d_5000x3_k20": dict(profile=4, uep=2, tile=(5000, 3)), "2d_1x9_k20": dict(profile=4, uep=2, tile=(1, 9))})
# frames and raw words in total a configuration's sweep may hold, by its number of distinct codes (measured: one code 851 .. 1319 frames
# and 1.7 .. 2.9 M words, two codes up to 1724 and 3.8 M, four codes 2575 and 5.8 M)
BUDGET = {1: (1400, 3_000_000), 2: (1800, 4_000_000), 4: (2800, 6_500_000)}


def steps(count):
    """[(W, one_launch)] -> the W at which the tile count differs from that of W - 1, over the W the plan serves in one launch."""
    out, prev = [], None
    for W in range(1, W_MAX + 1):
        c = count(W)
        if c is None:
            prev = None
            continue
        if prev is not None and c != prev:
            out.append(W)
        prev = c
    return out


def check_steps(found, lattice, what):
    assert len(found) >= 2, (what, found)
    have = set(lattice)
    for W in found:
        assert W in have and W - 1 in have, (what, W)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", rp.ONE_K)
def test_lattice_holds_every_step_of_the_batch_encoders(t3, name, mode):
    """tiles_per_frame of the batched single-k encoder, pixel and RGB front end (they may pick different tiles), COMPAT and FIXED.  The
    plan serves every FIXED frame in one launch; in COMPAT not the first 17 to 23 word counts, at which band 0 -- ceil(n_sym / 9) symbols, the
    longest band -- holds no whole block and the body is empty."""
    cfg = t3.make_cfg(mode=mode, **rp.CONFIGS[name])
    lat = fe.lattice_of(rp.CONFIGS[name])
    k = fe.band_codes(rp.CONFIGS[name])[0]
    empty = [W for W in range(1, W_MAX + 1) if -(-fe.n_sym(W) // 9) < k] if mode == 0 else []
    assert len(empty) == {0: 0, 24: 23, 22: 21, 20: 19, 18: 17}[k if mode == 0 else 0]
    for fmt in (t3.FRAMES_PIXELS, t3.FRAMES_RGB):
        plans = {W: t3.frames_plan(False, 2 * W, 2, cfg, fmt) for W in range(1, W_MAX + 1)}
        none = [W for W, p in plans.items() if not p.one_launch]
        assert none == empty, (name, mode, fmt, none[:30])
        check_steps(steps(lambda W: plans[W].tiles_per_frame if plans[W].one_launch else None), lat, (name, mode, fmt, "encode"))


@pytest.mark.parametrize("name", rp.ONE_K)
def test_lattice_holds_every_step_of_the_fused_decoder(t3, name):
    """FIXED: tiles_per_frame of the batched pixel decoder and n_tiles of the window plan (the fused decoder's tile range)."""
    cfg = t3.make_cfg(mode=1, **rp.CONFIGS[name])
    lat = fe.lattice_of(rp.CONFIGS[name])

    def dec(W):
        p = t3.frames_plan(True, 2 * W, 2, cfg, t3.FRAMES_PIXELS)
        return p.tiles_per_frame if p.one_launch else None

    def win(W):
        p = t3.window_plan(W, cfg, 2 * W, 1, 0, 0, 2 * W, 1)
        return p.n_tiles if p.tile_range else None
    check_steps(steps(dec), lat, (name, "decode"))
    check_steps(steps(win), lat, (name, "window"))


def test_recorded_steps(t3):
    """The steps measured when the lattice was designed, so that a planner that moves its tiles shows up here by name."""
    k20, k24 = rp.CONFIGS["k20"], rp.CONFIGS["k24"]
    enc = lambda kw, mode, fmt: steps(lambda W: (lambda p: p.tiles_per_frame if p.one_launch else None)(t3.frames_plan(False, 2 * W, 2, t3.make_cfg(mode=mode, **kw), fmt)))
    assert enc(k20, 1, t3.FRAMES_PIXELS) == [1143, 2285, 3427, 4570]
    assert enc(k20, 0, t3.FRAMES_PIXELS) == [1163, 2305, 3447, 4589]
    assert enc(k24, 1, t3.FRAMES_RGB) == [1396, 2792, 4188]
    assert steps(lambda W: t3.frames_plan(True, 2 * W, 2, t3.make_cfg(mode=1, **k20), t3.FRAMES_PIXELS).tiles_per_frame) == [1081, 2161, 3241, 4321]


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(ROOT, "tests", "golden", "enc_plan.json")) as f:
        return [g for g in json.load(f) if g["found"]]


def masked_codes(g):
    mask = int(g["case"].split("mask=")[1].split()[0], 16)
    return [g["band_k"][b] for b in range(9) if mask >> b & 1]


def test_recorded_tiles_rest_on_the_codes(recorded):
    """The invariant the lattice rests on: every recorded tile is 9 * Lq symbols with Lq a multiple of lcm(2, the codes of the launch's
    bands), so each of its multiples is a multiple of a subset unit of the frame's codes."""
    assert len(recorded) >= 90
    for g in recorded:
        ks = masked_codes(g)
        assert ks and g["Lq"] % fe.lcm(2, *ks) == 0, (g["case"], g["Lq"], ks)
        assert 9 * g["Lq"] % (9 * fe.lcm(2, *ks)) == 0 and 9 * fe.lcm(2, *ks) in fe.subset_units(g["band_k"]), g["case"]


def test_lattice_brackets_every_recorded_tile(recorded):
    """Every multiple of every recorded tile up to CAP has the whole bracket around it in the lattice of that frame's codes: at least one
    multiple per record, at least three per matrix-core (MfmaK, Uep) record."""
    lats = {}
    for g in recorded:
        ks = tuple(g["band_k"])
        have = lats.setdefault(ks, set(fe.lattice(ks)))
        tile = 9 * g["Lq"]
        mult = list(range(tile, fe.CAP + 1, tile))
        assert len(mult) >= (3 if g["kind"] in ("MfmaK", "Uep") else 1), (g["case"], tile)
        for S in mult:
            for d in range(fe.BRACKET[0], fe.BRACKET[1] + 1):
                assert fe.w_le(S) + d in have, (g["case"], S, d)
            assert fe.n_sym(fe.w_le(S)) <= S < fe.n_sym(fe.w_le(S) + 1)


def test_lattice_parts():
    """The dense run, the pad pixel alternating along the list, the 2-D units, the beacon run."""
    for name, kw in ENCODER_CONFIGS.items():
        lat = fe.lattice_of(kw)
        assert lat == sorted(set(lat)) and lat[: fe.DENSE + 1] == list(range(fe.DENSE + 1)), name
        assert lat[-1] <= W_MAX, name
        assert [fe.pixel_count(W, i) for i, W in enumerate(lat[:4])] == [0, 1, 4, 5]
        have = set(lat)
        if kw["profile"] == 4:
            tw, th = kw["tile"]
            for u in (tw, tw * th):
                for j in (1, 2, 3):
                    if u * j <= fe.CAP:
                        assert {fe.w_le(u * j), fe.w_le(u * j) + 1} <= have, (name, u, j)
        if kw.get("beacon"):
            w0 = fe.w_le(27 * fe.lcm(2, *fe.band_codes(kw)))
            assert set(range(w0, w0 + fe.BEACON_RUN)) <= have, name


def test_sweep_stays_within_its_budget():
    for name, kw in ENCODER_CONFIGS.items():
        lat = fe.lattice_of(kw)
        frames, words = BUDGET[len(set(fe.band_codes(kw)))]
        assert len(lat) <= frames and sum(lat) <= words, (name, len(lat), sum(lat))
