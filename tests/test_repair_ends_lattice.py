"""CPU proofs for tests/repair_ends.py, which tests/test_gpu_repair_ends.py sweeps the in-place repairs over: the lattice holds both
sides of every step of a repair launch's tile count (the library's host-only planners say where the steps are; the lattice is built
without them), the streams reach what they are aimed at -- stated on the streams and the yardsticks' answers alone --, and the
yardsticks' answers are fixed points that the oracle's frame decoder agrees with."""
import collections

import numpy as np
import pytest

import erasure_patterns as ep
import frame_ends as fe
import repair_ends as re
import rs_patterns as rp
from test_repair_semantics import E_RS, FUSED, GENERIC, SWEEP, expected, oracle_answer

W_MAX = fe.w_le(fe.CAP) + 1
NO_SLOT_IN_TAIL = ("k20_beacon83",)              # no frame up to W_MAX words ends in front of a beacon slot (profiles/repair_ends/notes.md)
# frames, raw words in total and flagged blocks in total a configuration's sweep may hold, by its number of distinct codes (measured:
# one code 235 .. 289 frames, 85 k .. 112 k words, 2.8 k .. 3.9 k flagged blocks; two codes 334 frames, 155 k words, 4.5 k flagged
# blocks; four codes 501 frames, 289 k words, 6.8 k flagged blocks)
BUDGET = {1: (320, 125_000, 4_400), 2: (370, 175_000, 5_000), 4: (560, 320_000, 7_600)}
FLAGGED_PER_FRAME = 27                           # at most three blocks a band carry a kind


def steps(count, n=re.STEPS):
    """The first n raw-word counts W at which count(W) differs from count(W - 1)"""
    out, prev = [], count(1)
    for W in range(2, W_MAX + 1):
        c = count(W)
        if c != prev:
            out.append(W)
            if len(out) == n:
                break
        prev = c
    return out


# ---- the plan's steps -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SWEEP)
def test_lattice_holds_the_first_steps_of_the_repair_plans(t3, name):
    """n_tiles of t3hip_repair_plan and tiles_per_frame of t3hip_repair_frames_plan: W and W - 1 of each of the first three steps are in
    the lattice; every lattice size plans (no refusal) on the path test_repair_semantics names."""
    cfg = t3.make_cfg(mode=1, **rp.CONFIGS[name])
    lat = re.repair_lattice(name); have = set(lat)
    assert list(lat) == sorted(have) and lat[0] == 1 and lat[: fe.DENSE] == tuple(range(1, fe.DENSE + 1)) and lat[-1] <= W_MAX
    for what, count in (("repair_plan", lambda W: t3.repair_plan(W, cfg).n_tiles), ("repair_frames_plan", lambda W: t3.repair_frames_plan(W, 3, cfg).tiles_per_frame)):
        found = steps(count)
        assert len(found) == re.STEPS, (name, what, found)
        for W in found:
            assert W in have and W - 1 in have, (name, what, W)
    for W in lat:                                                            # (a refusal raises T3Error)
        p = t3.repair_plan(W, cfg); fp = t3.repair_frames_plan(W, 3, cfg)
        assert p.path == fp.path == fp.one_launch == (1 if name in FUSED else 0), (name, W)
        assert p.n_tiles == fp.tiles_per_frame >= 1 and p.blocks_per_tile == (9 * re.FUSED_ROWS if p.path else re.GENERIC_BLOCKS), (name, W)


def test_recorded_steps(t3):
    """The steps measured when the lattice was designed, so that a planner that moves its tiles shows up here by name."""
    first = lambda name: steps(lambda W: t3.repair_plan(W, t3.make_cfg(mode=1, **rp.CONFIGS[name])).n_tiles)
    assert first("k20") == re.fused_steps(20) == [1081, 2161, 3241]
    assert first("k24") == re.fused_steps(24) == [1297, 2593, 3889]
    assert first("four_codes") == re.generic_steps("four_codes") == [604, 1226, 1845]
    assert first("k20_beacon83") == re.generic_steps("k20_beacon83") == [583, 1165, 1766]
    assert first("k22_beacon2_slot8") == re.generic_steps("k22_beacon2_slot8") == [641, 1281, 1943]


def test_slot_in_tail_frames():
    """The frames whose tail holds a beacon slot: three in a row for the slot-8 framing (the body ends within the last word's first
    eight bytes), none for the period-83 framing -- recorded, so that a change of either shows."""
    assert re.slot_in_tail("k22_beacon2_slot8") == (46, 47, 48)
    assert all(re.slot_in_tail(n) == () for n in NO_SLOT_IN_TAIL) and re.slot_in_tail("k20") == ()


# ---- what the streams reach -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SWEEP)
def test_streams_reach_the_frame_ends(orc, name):
    cs = re.cases(name)
    assert [c.W for c in cs] == list(re.repair_lattice(name))
    codes = set(fe.band_codes(rp.CONFIGS[name]))
    tail_lens = collections.Counter(); low = high = slot_frames = far_with_tail = 0
    seen = {k: set() for k in codes}; accepted = refused = 0
    frames = words = flagged = 0
    for c in cs:
        fr, rec = c.fr, c.rec
        assert fr.n_raw == c.W and fr.n_px == fe.pixel_count(c.W, c.i) and len(rec) == 9 * int(fr.L.out_words), (name, c.W)
        hs = int(fr.L.header_syms)
        assert np.array_equal(rec[:hs], fr.clean.reshape(-1)[:hs]), (name, c.W, "the header stays clean")
        tail, slots = re.tail_parts(fr.L, fr.ocfg)
        tail_lens[len(tail)] += 1
        slot_frames += 1 if len(slots) else 0
        for exp in (c.plain, c.era):                                         # every dirty tail byte has to change
            assert (rec[tail] != exp[tail]).all() and not exp[tail].any(), (name, c.W)
        low += int(((rec[tail] >= 1) & (rec[tail] <= 26)).sum()); high += int((rec[tail] > 26).sum())
        at = rp.beacon_index(fr.L, fr.ocfg)
        if len(at):
            assert rec[at[-1]] != c.era[at[-1]] and np.array_equal(c.era[at], fr.clean.reshape(-1)[at]) and np.array_equal(c.plain[at], c.era[at]), (name, c.W)
        far_with_tail += 1 if c.far and len(tail) else 0
        if c.far:
            assert c.plain_words[0] >= 1 and c.era_words[1] >= 1, (name, c.W)
        # the last block of every band: its (erased, wrong) pair as the stream shows it, and what the erasure yardstick did to it
        B = rp.block_index(fr.L, fr.ocfg); f0 = rp.band_first_block(fr.L); clean = fr.clean.reshape(-1)
        for b in range(9):
            if not fr.blocks[b]:
                continue
            idx = B[f0[b] + fr.blocks[b] - 1]
            hi = rec[idx] > 26
            seen[fr.ks[b]].add((int(hi.sum()), int(((rec[idx] != clean[idx]) & ~hi).sum())))
            if hi.any():
                ok = bool((c.era[idx] <= 26).all())
                assert ok or np.array_equal(c.era[idx], rec[idx]), (name, c.W, b)
                accepted += ok; refused += not ok
        assert c.era_words[4] <= FLAGGED_PER_FRAME, (name, c.W, c.era_words)
        frames += 1; words += c.W; flagged += c.era_words[4]
    for n in range(1, 9):
        assert tail_lens[n] >= 3, (name, "tail length", n, sorted(tail_lens.items()))
    assert low > 0 and high > 0, (name, low, high)
    if rp.CONFIGS[name].get("beacon"):
        assert slot_frames >= re.SLOT_FRAMES or (name in NO_SLOT_IN_TAIL and slot_frames == 0), (name, slot_frames)
    for k in codes:
        assert seen[k] >= set(ep.admissible(k)) | set(ep.beyond(k)), (name, k, sorted((set(ep.admissible(k)) | set(ep.beyond(k))) - seen[k]))
    assert accepted > 0 and refused > 0 and far_with_tail > 0, (name, accepted, refused, far_with_tail)
    print("%s: %d frames, %d words, %d flagged blocks, non-beacon tail lengths %s, %d frames with a beacon slot in the tail"
          % (name, frames, words, flagged, sorted(tail_lens.items()), slot_frames))
    cap = BUDGET[len(codes)]
    assert frames <= cap[0] and words <= cap[1] and flagged <= cap[2], (name, frames, words, flagged)


# ---- the yardsticks ---------------------------------------------------------------------------------------------------------------------
def test_syndromes_of_a_few_rows_are_the_loop_s(orc):
    """rs_patterns.Field.syndromes takes a short cut for fewer than Field.SMALL rows (a sweep asks for the syndromes of a block or a band
    some 10^5 times): the same numbers as the loop over positions, for every R and every row count around the switch; every symbol
    value at every position is among the rows."""
    F = rp.field(orc)
    rng = np.random.default_rng(20261020)
    every = np.zeros((26 * 27, 26), np.uint8); i = np.arange(26 * 27); every[i, i // 27] = i % 27
    for R in (2, 4, 6, 8):
        for n in (0, 1, 2, 9, F.SMALL - 1, F.SMALL, F.SMALL + 1):
            rows = rng.integers(0, 27, (n, 26), dtype=np.uint8)
            a, b, c = F.syndromes_loop(rows, R), F.syndromes_small(rows, R), F.syndromes(rows, R)
            assert a.dtype == b.dtype == c.dtype == np.uint8 and a.shape == b.shape == c.shape == (n, R)
            assert np.array_equal(a, b) and np.array_equal(a, c), (R, n)
        assert np.array_equal(F.syndromes_loop(every, R), F.syndromes_small(every, R)), R


@pytest.mark.parametrize("name", SWEEP)
def test_yardsticks_on_the_streams(orc, name):
    """Both answers are fixed points; the oracle's frame decoder gives the received stream and the plain answer one verdict (and, where
    nothing is refused, the same pixels); on a stream without a flagged block the two yardsticks agree."""
    for c in re.cases(name):
        fr = c.fr; tag = (name, c.W)
        M = c.plain_words[0]
        exp2, words2, _ = expected(orc, fr, c.plain)
        assert np.array_equal(exp2, c.plain) and words2 == [M, 0, 0], tag
        w = c.era_words
        exp2, words2, _ = ep.expected_erasures(orc, fr, c.era)
        assert np.array_equal(exp2, c.era) and words2 == [0, w[1], 0, 0, w[4] - w[5], 0], tag
        assert w[0] == 0 and w[5] <= w[4] and w[1] >= w[4] - w[5], tag
        if c.i % 10 == 0:
            a, b = oracle_answer(orc, c.rec), oracle_answer(orc, c.plain)
            assert a[0] == b[0] == (E_RS if M else 0), tag
            if not M:
                assert np.array_equal(a[1], b[1]), tag
            B = rp.block_index(fr.L, fr.ocfg)
            low = c.rec.copy(); low[B] %= 27                                 # no body block is flagged: the erasure rule is the plain rule
            p, pw, _ = expected(orc, fr, low)
            e, ew, _ = ep.expected_erasures(orc, fr, low)
            assert np.array_equal(p, e) and ew == [0] + pw + [0, 0], tag
            assert pw[0] == M and np.array_equal(p % 27, c.plain % 27), tag  # (the plain rule reads bytes mod 27)
