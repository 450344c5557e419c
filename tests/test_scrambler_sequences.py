"""CPU proofs under tests/test_gpu_scrambler.py: the scrambler's whole sequence space (tests/scrambler_seqs.py), the library's host side
on all of it, and the oracle's answer to every damaged frame the GPU tests decode.

The kernels read ScrCycle, never the recurrence; what the GPU tests compare them with is the oracle's stream.  Here: the recurrence
restated in Python, the oracle's scramble, the reference's (where oracle/_ref is built) and t3hip_scramble_symbol give the same states
for all 81 (next-map, start state) pairs and both representatives of every class; there are 21 classes; the six transient ones are
exactly those whose first state is not the 6-periodic tail continued backwards, and they need uint32 wrap-around; the header carries
the seeds mod 27 and, in FIXED, the next-map itself."""
import ctypes as C

import numpy as np
import pytest

import frame_ends as fe
import oracle_lib as ol
import rs_patterns as rp
import scrambler_seqs as ss
from test_repair_semantics import FUSED, SWEEP, expected as repair_expected

N_STATES = 64
ALL_SEEDS = tuple(ss.ALL81) + ss.REPS + ss.REPS2
DEC_FRAMINGS = tuple(rp.CONFIGS)


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    return ge.load_package()


def states_of(scramble, seed, n=N_STATES):
    """The states a scramble function adds: it is run on zeros, so each output symbol is (st, st, st) = 13 st."""
    out = np.asarray(scramble(np.zeros(n, np.uint8), *seed))
    assert (out % 13 == 0).all()
    return (out // 13).tolist()


# ---- the sequence space ---------------------------------------------------------------------------------------------------------------
def test_restatement_oracle_and_reference_agree(orc):
    refs = [ol.Ref()] if ol.have_ref() else []
    for seed in ALL_SEEDS:
        want = ss.scr_states(*seed, N_STATES)
        assert states_of(orc.scramble, seed) == want, seed
        for r in refs:
            assert states_of(r.scramble, seed) == want, seed
        m = ss.next_map(seed[0], seed[1]); st = seed[2] % 3; model = []             # the map model: next-map and start state
        for _ in range(N_STATES):
            st = m[st]; model.append(st)
        assert model == want, seed
        sy = np.arange(N_STATES, dtype=np.uint8) % 27                               # ... and the symbols, both directions
        fwd = orc.scramble(sy, *seed)
        assert np.array_equal(fwd, ss.scramble(sy, *seed)) and np.array_equal(orc.scramble(fwd, *seed, 1), sy), seed
        assert np.array_equal(ss.scramble(fwd, *seed, inverse=True), sy), seed


def test_twenty_one_classes():
    assert len(ss.MAPS) == 27 and len(ss.ALL81) == 81 and len(set(ss.ALL81)) == 81
    assert sorted(ss.MAPS) == sorted((x, y, z) for x in range(3) for y in range(3) for z in range(3))
    for m, (a, b) in ss.MAPS.items():
        assert ss.next_map(a, b) == m and a in ss.CAND and b in ss.CAND
        affine = any(all((p * s + q) % 3 == m[s] for s in range(3)) for p in range(3) for q in range(3))
        assert ss.wraps(a, b) == (not affine), (m, a, b)                              # a pair without wrap-around wherever one exists
    seqs = {tuple(ss.scr_states(*s, N_STATES)) for s in ss.ALL81}
    assert len(seqs) == len(ss.SEQUENCES) == 21
    kinds = [s.kind for s in ss.SEQUENCES]
    assert {k: kinds.count(k) for k in set(kinds)} == {"constant": 3, "period2": 6, "period3": 6, "transient": 6}
    for i, s in enumerate(ss.SEQUENCES):
        for rep in (s.rep, s.rep2):
            assert tuple(ss.scr_states(*rep, 8)) == s.states and ss.class_of(rep) == i
        assert s.rep[:2] == s.rep2[:2] and s.rep2[2] % 3 == s.rep[2] and s.rep2[2] >= ss.M32 - 3 and s.rep[2] < 3
        assert s.rep2[2] % 27 != s.rep[2]                                             # the header's % 27 sees another number
        full = ss.scr_states(*s.rep, N_STATES)
        tail_backwards = full[6]                                                     # cyc[4]: the 6-periodic tail continued to index 0
        assert (full[0] != tail_backwards) == (s.kind == "transient"), s
        assert full[1] == full[7] and full[2:8] == full[8:14], s                       # pre[1] never differs; the tail is 6-periodic
        assert (full[0] != full[2]) == (s.kind in ("transient", "period3")), s
        assert (full[0] != full[3]) == (s.kind in ("transient", "period2")), s        # who sees a phase that is off by three
        if s.kind == "transient":
            assert s.wrap and full[0] != full[1] and set(full[1:]) == {full[1]}, s
            assert all(ss.wraps(a, b) for (a, b, s0) in ss.ALL81 if tuple(ss.scr_states(a, b, s0, 8)) == s.states)
    assert ss.classes(ss.ALL81) == ss.classes(ss.REPS) == ss.classes(ss.REPS2) == list(range(21))
    assert (1, 1, 1) in ss.ALL81 and ss.SEQUENCES[ss.class_of((1, 1, 1))].states[:6] == (2, 0, 1, 2, 0, 1)


# ---- the library's host side ----------------------------------------------------------------------------------------------------------
def test_host_scramble_symbol(built, orc):
    L = built.lib()
    L.t3hip_scramble_symbol.restype = C.c_uint8
    sy = (np.arange(N_STATES) * 7 % 27).astype(np.uint8)
    for seed in ALL_SEEDS:
        a, b, s0 = seed
        for inverse in (0, 1):
            st = C.c_uint32(s0 % 3); got, states = [], []
            for x in sy:
                got.append(L.t3hip_scramble_symbol(C.c_uint8(int(x)), C.c_uint32(a), C.c_uint32(b), C.byref(st), C.c_int(inverse)))
                states.append(st.value)
            assert states == ss.scr_states(*seed, N_STATES), (seed, inverse)
            assert np.array_equal(np.array(got, np.uint8), orc.scramble(sy, a, b, s0, inverse)), (seed, inverse)


@pytest.mark.parametrize("mode", [0, 1])
def test_host_header(built, orc, mode):
    t3 = built
    raw = np.zeros((1, 9), np.uint8)
    for seed in ALL_SEEDS:
        for name in ("k20", "four_codes"):
            kw = dict(rp.CONFIGS[name], seed=seed)
            cfg, ocfg = t3.make_cfg(mode=mode, **kw), ol.make_cfg(mode=mode, **kw)
            rc, s = orc.encode_profile(raw, ocfg); assert rc == 0
            hdr = t3.header_encode(cfg, 1)
            assert len(hdr) == int(t3.plan(1, cfg).header_syms) == (90 if mode else 52)
            assert np.array_equal(hdr, s.reshape(-1)[: len(hdr)]), (seed, name, mode)
            hp = t3.header_pack(cfg)
            assert np.array_equal(hp, orc.header_pack(ocfg)) and np.array_equal(hp[:18], hdr[:18]) and np.array_equal(hp[18:], hdr[26:35])
            mod27 = tuple(x % 27 for x in seed)
            assert tuple(hp[9:12]) == mod27
            mine, theirs = t3.header_unpack(hp)[0], orc.header_unpack(hp)[0]
            assert (mine.seed_a, mine.seed_b, mine.seed_s0) == (theirs.seed_a, theirs.seed_b, theirs.seed_s0) == mod27, seed
            if mode == 1:
                m = ss.next_map(seed[0], seed[1])
                assert hdr[69] == m[0] + 3 * m[1] + 9 * m[2], (seed, hdr[69], m)            # ext[26], the last data symbol of block 3
                seen = ol.make_cfg(mode=1)
                rc, _ = orc.decode_frame(s, seen)
                assert rc == 0 and (seen.seed_a, seen.seed_b, seen.seed_s0) == mod27, seed


# ---- the frames of the GPU tests ------------------------------------------------------------------------------------------------------
def check_frame(orc, fr):
    """The oracle's decode of both damaged streams of a DecFrame: le_t gives the frame, far is refused because of exactly one block."""
    bad = fr.le_t()
    assert not np.array_equal(bad, fr.clean)
    e00 = fr.errors()[0][0]; t = rp.tparam(fr.ks[0])
    assert (e00 != 0).sum() == t and (e00[fr.seed % 2] if t == 1 else e00[0] and e00[1])    # a correction at body symbols 0 and 1
    seen = ol.make_cfg(mode=1)
    rc, px = orc.decode_frame(bad, seen)
    assert rc == 0 and np.array_equal(px, fr.padded), (fr.name, fr.size, fr.scr)
    assert (seen.seed_a, seen.seed_b, seen.seed_s0) == tuple(x % 27 for x in fr.scr)
    tight = fr.tight()
    rc, px = orc.decode_frame(tight, ol.make_cfg(mode=1))
    assert rc == 0 and np.array_equal(px, fr.padded), (fr.name, fr.size, fr.scr, "tight")
    B0 = rp.block_index(fr.L, fr.ocfg)[0]
    d0 = np.flatnonzero(tight.reshape(-1)[B0] != fr.clean.reshape(-1)[B0])
    assert d0.tolist() == list(range(2, 2 + t)), (fr.name, d0)                               # t errors, none at body symbols 0 and 1
    far = fr.far()
    assert orc.decode_frame(far, ol.make_cfg(mode=1))[0] == -6, (fr.name, fr.size, fr.scr)
    B = rp.block_index(fr.L, fr.ocfg)
    row = rp.field(orc).sub[far.reshape(-1)[B[0]], fr.clean.reshape(-1)[B[0]]]             # the one block the two streams differ in
    diff = np.flatnonzero((far != bad).reshape(-1))
    assert len(diff) and set(diff.tolist()) <= set(B[0].tolist())
    _, _, ok = orc.rs_decode_blocks(fr.ks[0], row[None, :], mode=1)
    assert ok[0] == 0 and not rp.is_codeword(orc, fr.ks[0], row[None, :])[0]                # ... does not decode: the verdict counts 1


@pytest.mark.parametrize("name", DEC_FRAMINGS)
def test_oracle_decodes_the_gpu_frames(built, orc, name):
    """Every (framing, size, seed) the single-frame cells of test_gpu_scrambler.py decode (content salt 0; the further contents of the
    batches and the image frames follow below): the errors are within t per block (the oracle gives the frame back), the far block is
    uncorrectable and the only one."""
    for size in ss.SIZES:
        for fr in ss.dec_frames(built, name, size, ss.seeds_at(size)):
            check_frame(orc, fr)


@pytest.mark.parametrize("name", SWEEP)
def test_repair_yardstick(built, orc, name):
    """scrambler_seqs.repair_want (the clean stream, the far block as received, counts from the bytes that differ) is what
    test_repair_semantics.expected gives for both damaged streams.  Errors are additive on the wire whatever the scrambler adds, so the
    two small sizes stand for the rest."""
    for size, seeds in (("w2", ss.REPS2), ("tile", ss.REPS)):
        for fr in ss.dec_frames(built, name, size, seeds):
            for s, far in ((fr.le_t(), []), (fr.tight(), []), (fr.far(), [(0, 0)])):
                exp, words, where = repair_expected(orc, fr, s)
                mine, my_words = ss.repair_want(fr, s, far)
                assert where == far and words == my_words and np.array_equal(exp, mine), (name, size, fr.scr)


@pytest.mark.parametrize("name", ss.BATCH_DEC)
def test_oracle_decodes_the_batch_frames(built, orc, name):
    """test_gpu_scrambler.test_batched_decoders decodes three contents per seed (scrambler_seqs.batch_sets): salt 0 is among the frames
    above; here the other two, all three streams of each -- the far stream of salt 1 and the tight one of salt 2, which the batch takes
    (scrambler_seqs.batch_streams), among them."""
    for size, seeds in ss.BATCH_SIZES:
        sets = ss.batch_sets(built, name, size, seeds)
        assert [fr.scr for fr in sets[0]] == [tuple(s) for s in seeds] and len({fr.seed for x in sets for fr in x}) == 3
        for frs in zip(*sets):
            coded = ss.batch_streams(frs)
            assert np.array_equal(coded[1], fe.u8(frs[1].far())) and np.array_equal(coded[2], fe.u8(frs[2].tight()))
            assert not np.array_equal(frs[0].padded, frs[1].padded) and not np.array_equal(frs[1].padded, frs[2].padded)
            for fr in frs[1:]:
                check_frame(orc, fr)


def test_oracle_decodes_the_image_frames(built, orc):
    """The frames of test_gpu_scrambler.test_image_batches, all three under every representative: frames 0 and 2 decode to their pixels,
    frame 1 is refused, and is the clean frame but for its first block, which does not decode."""
    ic = ss.image_case(built)
    ic.prefetch(ss.REPS)
    L = built.plan(ic.n_raw, built.make_cfg(mode=1, **ss.IMG_KW))
    B0 = rp.block_index(L, ol.make_cfg(mode=1, **ss.IMG_KW))[0]

    def one(seed):
        bad, clean = ic.damaged(seed), ic.coded(seed)
        for f in (0, 2):
            rc, px = orc.decode_frame(bad[f].reshape(-1, 9), ol.make_cfg(mode=1))
            assert rc == 0 and np.array_equal(px, ic.px[f]), (seed, f)
            d0 = np.flatnonzero(bad[f][B0] != clean[f][B0])
            assert d0.tolist() == ([0, 1, 2], None, [2, 3, 4])[f] and (bad[f] != clean[f]).sum() == 3, (seed, f, d0)
        assert orc.decode_frame(bad[1].reshape(-1, 9), ol.make_cfg(mode=1))[0] == -6, seed
        diff = np.flatnonzero(bad[1] != clean[1])
        assert len(diff) and set(diff.tolist()) <= set(B0.tolist()), seed
        row = rp.field(orc).sub[bad[1][B0], clean[1][B0]]
        assert orc.rs_decode_blocks(20, row[None, :], mode=1)[2][0] == 0 and not rp.is_codeword(orc, 20, row[None, :])[0], seed
        return seed

    assert ss.classes(ss._pool(one, ss.REPS)) == list(range(21))


# ---- the plans the GPU tests rest on (host arithmetic, no device) ---------------------------------------------------------------------
def test_plans(built):
    """What routes a frame to a launch with a `first` / pre-period form, as the library's planners say it, for every framing, size and
    sequence class (the plans do not depend on the seed: asserted by running all of them).  scrambler_seqs.TILE_RANGE is the
    expectation: FIXED, one k, 1-D, no beacon is what the fused pixel kernel takes with a tile range and what a batch decodes in one
    launch -- exactly the framings plan_fixed_fused takes without a beacon.  The split of the others between the one-launch UEP and the
    two-kernel decoder has no host entry; it shows in which cells fail under a wrong first-block row (profiles/scrambler/notes.md)."""
    t3 = built
    assert [n for n in rp.CONFIGS if ss.TILE_RANGE[n]] == list(rp.ONE_K) and not any(ss.TILE_RANGE[n] for n in ss.ENC_EXTRA)
    for name, kw in ss.ENC_FRAMINGS.items():
        tr = ss.TILE_RANGE[name]
        for size, (W, n_px) in ss.frame_sizes(kw).items():
            for seed in ss.seeds_at(size):
                tag = (name, size, seed)
                for mode in (0, 1):                                                  # batch encode: pixels and RGB in one launch, raw words never
                    cfg = t3.make_cfg(mode=mode, **dict(kw, seed=seed))
                    for fmt, f, n in ((t3.FRAMES_PIXELS, "pixels", n_px), (t3.FRAMES_RGB, "rgb", n_px), (t3.FRAMES_WORDS, "words", W)):
                        want = ss.batch_encode_one_launch(name, mode, size, f)
                        assert want is None or t3.frames_plan(False, n, 3, cfg, fmt).one_launch == want, (tag, mode, f)
                    assert ss.batch_encode_one_launch(name, mode, size, "pixels") == tr or (mode == 0 and size in ("w1", "w2"))
                if name not in rp.CONFIGS:
                    continue
                cfg = t3.make_cfg(mode=1, **dict(kw, seed=seed))
                assert t3.frames_plan(True, 2 * W, 3, cfg, t3.FRAMES_PIXELS).one_launch == tr, tag
                assert t3.frames_plan(True, 2 * W, 3, cfg, t3.FRAMES_RGB).one_launch == tr, tag
                assert t3.frames_plan(True, W, 3, cfg, t3.FRAMES_WORDS).one_launch == 0, tag
                assert t3.frames_plan(True, 2 * W, 1, cfg, t3.FRAMES_PIXELS).one_launch == 0, tag
                if name in SWEEP:
                    assert t3.repair_plan(W, cfg).path == (1 if name in FUSED else 0), tag
                for label, win in ss.windows_of(2 * W):
                    p = t3.window_plan(W, cfg, *win)
                    assert p.tile_range == tr, (tag, label)
                    fp = t3.frames_window_plan(W, 3, cfg, *win, t3.WINDOW_PIXELS)
                    assert fp.one_launch == tr and (fp.win.tile_lo, fp.win.tile_hi) == (p.tile_lo, p.tile_hi), (tag, label)
                    if tr:
                        assert p.tile_hi > p.tile_lo and (p.tile_lo >= 1) == ss.starts_behind_tile0(name, size, label), (tag, label, p.tile_lo)
                        if size == "cap":
                            assert p.n_tiles >= 3 and (label != "last" or p.tile_hi == p.n_tiles) and (label != "whole" or p.tile_hi == p.n_tiles)
                        if label == "first":
                            assert p.tile_lo == 0 and p.tile_hi == 1, (tag, p.tile_hi)
                    assert ss.far_verdict(name, size, label) == ([0, 0] if (p.tile_range and p.tile_lo >= 1) else [0, 1]), (tag, label)
    cfg = t3.make_cfg(mode=1, **ss.IMG_KW)                                            # the image front end: S15 frames, one launch each way
    assert t3.frames_plan(False, 854 * 480, 3, cfg, t3.FRAMES_RGB).one_launch == 1
    assert t3.frames_window_plan(854 * 480 // 2, 3, cfg, 854, 480, 0, 0, 854, 480, t3.WINDOW_RGB).one_launch == 1
