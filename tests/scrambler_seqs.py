"""Every sequence the scrambler can produce, and the frames that carry them through the codec (helper module, no tests).

The scrambler steps its state before each use: st <- ((a * st + b) mod 2^32) mod 3, from st = s0 mod 3 (ternary_image_codec_v6_min.hpp:81-94,
943, 1116; t3o_scramble).  The state a step starts from is one of 0, 1, 2, so a seed (a, b) acts through its next-map
(next[0], next[1], next[2]) -- one of 27 -- and the start state.  scr_states() below does not use that model: it runs the recurrence in
uint32 arithmetic; tests/test_scrambler_sequences.py proves the two, the oracle and the library's host side equal.

  MAPS        next-map -> one (a, b) that realises it: without uint32 wrap-around where one exists (the nine affine maps), else from the
              candidate set CAND (found by search when the module is imported)
  ALL81       every (a, b, s0) of MAPS x s0 in 0, 1, 2
  SEQUENCES   the distinct state sequences of ALL81 -- 21 classes: 3 constant, 6 of period 2, 6 of period 3 and 6 transient ones
              x, y, y, y, ... (x != y); each with a representative and a second one whose s0 is s0 + 3 j in 2^32 - 3 .. 2^32 - 1
  REPS, REPS2 the two representatives of every class, in the order of SEQUENCES

The library's kernels never run the recurrence: they read ScrCycle (two pre-period states and a 6-periodic tail).  Only a transient
sequence has pre[0] different from the tail continued backwards, and only a sequence of period 2 or a transient one tells a phase that is
off by three from the right one.

Frames: frame_sizes() picks four sizes per framing from frame_ends.lattice_of; EncCase holds one content (RGB, its pixels, its raw words)
and the oracle's stream of it per seed; DecFrame is rs_patterns.Frame under a seed with the two damaged streams the decoder tests use."""
import collections
import functools
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import frame_ends as fe
import oracle_lib as ol
import rs_patterns as rp

M32 = 1 << 32
CAND = tuple(range(6)) + tuple(range(1 << 31, (1 << 31) + 3)) + tuple(range(M32 - 3, M32))


def scr_states(a, b, s0, n):
    """The first n states the scrambler uses, by the recurrence itself (uint32 product and sum, then mod 3; stepped before use)."""
    st = s0 % 3
    out = []
    for _ in range(n):
        st = ((a * st + b) % M32) % 3
        out.append(st)
    return out


def scramble(syms, a, b, s0, inverse=False):
    """scramble_symbol / descramble_symbol over a run of symbols: the state added to (subtracted from) each of the three trits."""
    s = np.asarray(syms, np.int64)
    st = np.array(scr_states(a, b, s0, len(s)), np.int64)
    if inverse:
        st = 3 - st
    return sum((((s // 3 ** i) % 3 + st) % 3) * 3 ** i for i in range(3)).astype(np.uint8)


def next_map(a, b):
    return tuple(((a * s + b) % M32) % 3 for s in range(3))


def wraps(a, b):
    """Does a * st + b leave uint32 for some state?"""
    return 2 * a + b >= M32


def _maps():
    found = {}
    for a in range(6):                                                      # no wrap-around: the affine maps
        for b in range(6):
            found.setdefault(next_map(a, b), (a, b))
    for a in CAND:
        for b in CAND:
            found.setdefault(next_map(a, b), (a, b))
    return {m: found[m] for m in sorted(found)}


MAPS = _maps()
ALL81 = tuple((a, b, s0) for (a, b) in MAPS.values() for s0 in range(3))

Seq = collections.namedtuple("Seq", "kind states rep rep2 wrap")


def kind_of(states):
    s = list(states)
    if len(set(s)) == 1:
        return "constant"
    if s[0] != s[2] and s[1:] == [s[1]] * (len(s) - 1):
        return "transient"
    if s[:-2] == s[2:]:
        return "period2"
    if s[:-3] == s[3:]:
        return "period3"
    raise AssertionError(s)


def _sequences():
    by = {}
    for (a, b, s0) in ALL81:
        by.setdefault(tuple(scr_states(a, b, s0, 8)), []).append((a, b, s0))
    out = []
    for states in sorted(by):
        seeds = sorted(by[states], key=lambda s: (wraps(s[0], s[1]), s))       # a seed without wrap-around where the class has one
        a, b, s0 = seeds[0]
        big = next(x for x in range(M32 - 3, M32) if x % 3 == s0)
        out.append(Seq(kind_of(states), states, (a, b, s0), (a, b, big), all(wraps(x[0], x[1]) for x in by[states])))
    return tuple(out)


SEQUENCES = _sequences()
REPS = tuple(s.rep for s in SEQUENCES)
REPS2 = tuple(s.rep2 for s in SEQUENCES)
CLASS_OF = {s.states: i for i, s in enumerate(SEQUENCES)}


def class_of(seed):
    return CLASS_OF[tuple(scr_states(*seed, 8))]


def classes(seeds):
    """The sorted class numbers a list of seeds covers."""
    return sorted({class_of(s) for s in seeds})


def seeds_at(size):
    """The seeds a cell runs at a size: all 81 at the largest, the 21 representatives elsewhere (the second ones at W = 2)."""
    return ALL81 if size == "cap" else REPS2 if size == "w2" else REPS


# ---- sizes ---------------------------------------------------------------------------------------------------------------------------
SIZES = ("w1", "w2", "tile", "cap")
ENC_EXTRA = {"2d_5000x3_k20": dict(profile=4, uep=2, tile=(5000, 3)), "2d_1x9_k20": dict(profile=4, uep=2, tile=(1, 9))}
ENC_FRAMINGS = dict(rp.CONFIGS, **ENC_EXTRA)


def frame_sizes(kw):
    """size -> (raw words W, pixels): one word; two words, odd pixel count; the lattice entry right behind the first boundary of the fused
    decoder's tile (52 blocks per band, of the framing's shortest code), odd; the largest lattice entry (about frame_ends.CAP symbols: at
    least three tiles of every kernel, the last one ragged)."""
    Ws = fe.lattice_of(kw)
    S1 = 9 * 52 * min(fe.band_codes(kw))
    wt = fe.w_le(S1) + 1
    assert wt in Ws and fe.n_sym(wt) > S1 >= fe.n_sym(wt - 1) and 3 * 11232 < fe.n_sym(Ws[-1]) <= fe.CAP + 9
    return {"w1": (1, 2), "w2": (2, 3), "tile": (wt, 2 * wt - 1), "cap": (Ws[-1], 2 * Ws[-1])}


def _pool(fn, items):
    items = list(items)
    if not items:
        return []
    first = fn(items[0])                                                       # (the oracle builds its tables on first use)
    with ThreadPoolExecutor(fe.WORKERS) as ex:
        return [first] + list(ex.map(fn, items[1:]))


def _frozen(a):
    a = fe.u8(a).copy()
    a.setflags(write=False)
    return a


class EncCase:
    """One content of a framing at a size: RGB bytes, the pixels the bridge makes of them, their raw words; want(fe, seeds) -> the
    oracle's coded bytes per seed (encode_frame for the pixel and RGB front ends, encode_profile for the raw words)."""

    def __init__(self, name, mode, size, salt=0):
        self.name, self.mode, self.size = name, mode, size
        self.kw = ENC_FRAMINGS[name]
        self.W, self.n_px = frame_sizes(self.kw)[size]
        orc = ol.oracle()
        rng = np.random.default_rng([zlib.crc32(name.encode()), self.W, salt])
        self.rgb = _frozen(rng.integers(0, 256, 3 * self.n_px, dtype=np.uint8))
        self.px = orc.rgb_to_quant(self.rgb)
        self.raw = _frozen(orc.pack_pixels(self.px))
        self._want = {}

    def data(self, front_end):
        """(input bytes, units)"""
        return {"pixels": (fe.u8(self.px), self.n_px), "rgb": (self.rgb, self.n_px), "words": (self.raw, self.W)}[front_end]

    def _one(self, key):
        words, seed = key
        orc = ol.oracle(); cfg = ol.make_cfg(mode=self.mode, **dict(self.kw, seed=seed))
        rc, s = orc.encode_profile(self.raw.reshape(-1, 9), cfg) if words else orc.encode_frame(self.px, cfg, cap=self.n_px + 64)
        assert rc == 0, (self.name, self.mode, self.size, seed)
        return _frozen(s)

    def want(self, front_end, seeds):
        keys = [(front_end == "words", tuple(s)) for s in seeds]
        todo = [k for k in keys if k not in self._want]
        for k, s in zip(todo, _pool(self._one, todo)):
            self._want[k] = s
        return [self._want[k] for k in keys]


@functools.lru_cache(maxsize=8)
def enc_case(name, mode, size, salt=0):
    return EncCase(name, mode, size, salt)


# ---- damaged FIXED streams -----------------------------------------------------------------------------------------------------------
INJECT_SEED = 20261019


class DecFrame(rp.Frame):
    """rs_patterns.Frame of a framing at one of frame_sizes under a scrambler seed, with the two streams of the decoder tests:
      le_t   0 .. t errors in every block at the band's own t (the oracle's inject_errors on a zero band gives the additive rows), and in
             block 0 of band 0 rs_patterns.forced_first: t errors that include body symbols 0 and 1, the two pre-period states
      tight  the same with block 0 of band 0 holding t errors at positions 2 .. t + 1 instead: one wrong state at body symbol 0 or 1 is then
             more than the block's code corrects (under forced_first it would hide in a position that is in error anyway)
      far    the same with block 0 of band 0 replaced by a row that no codeword is within t of (one of rs_patterns.beyond_t's rows with syndromes (s, 0, .., 0))"""

    def __init__(self, plan, name, size, scr, salt=0):
        W, n_px = frame_sizes(rp.CONFIGS[name])[size]
        super().__init__(ol.oracle(), plan, name, n_px, SIZES.index(size) + 200 + 10 * salt, scr)
        self.size, self.scr = size, tuple(scr)
        assert self.n_raw == W and all(self.blocks)

    def errors(self):
        orc = self.orc; out = []
        for b in range(9):
            z = np.zeros((self.blocks[b], 26), np.uint8)
            e = orc.inject_errors(z, 0, self.blocks[b], INJECT_SEED + 16 * self.seed + b, rp.tparam(self.ks[b])).reshape(-1, 26)
            assert ((e != 0).sum(axis=1) <= rp.tparam(self.ks[b])).all()
            out.append(e)
        out[0][0] = rp.forced_first(self.ks[0], self.seed)
        return out

    def le_t(self):
        return rp.apply(self.orc, self.clean, self.L, self.ocfg, self.errors())

    def tight(self):
        e = self.errors()
        t = rp.tparam(self.ks[0])
        e[0][0] = 0
        e[0][0][2: 2 + t] = np.random.default_rng([self.seed, 7]).integers(1, 27, t)
        return rp.apply(self.orc, self.clean, self.L, self.ocfg, e)

    def far(self):
        e = self.errors()
        e[0][0] = rp.beyond_t(self.ks[0])["s0"][(class_of(self.scr) + self.seed) % 52]
        return rp.apply(self.orc, self.clean, self.L, self.ocfg, e)

    def want(self):
        """What a decode of le_t gives: (pixel bytes, raw-word bytes)"""
        return fe.u8(self.padded), fe.u8(self.orc.pack_pixels(self.padded))


def repair_want(fr, received, far=()):
    """What a repair leaves of a DecFrame's stream: the clean stream, the blocks of `far` [(band, block)] as received -> (bytes,
    [uncorrectable blocks, blocks changed, bytes changed]).  tests/test_scrambler_sequences.py holds it against test_repair_semantics.expected."""
    rec = fe.u8(received); out = fr.clean.reshape(-1).copy()
    B = rp.block_index(fr.L, fr.ocfg); f0 = rp.band_first_block(fr.L)
    for (b, m) in far:
        out[B[f0[b] + m]] = rec[B[f0[b] + m]]
    diff = out != rec
    return out, [len(far), int(diff[B].any(axis=1).sum()), int(diff[int(fr.L.header_syms):].sum())]


def dec_frames(t3, name, size, seeds, salt=0):
    """The DecFrames of a framing at a size, one per seed, built in the oracle pool (salt: another content, for batches)."""
    def plan_for(seed):
        cfg = t3.make_cfg(mode=1, **dict(rp.CONFIGS[name], seed=seed))
        return lambda n_raw: t3.plan(n_raw, cfg)
    return _pool(lambda seed: DecFrame(plan_for(seed), name, size, seed, salt), [tuple(s) for s in seeds])


BATCH_DEC = ("k20", "luma")                                              # the one-launch and the loop path of the batch decoders
BATCH_SIZES = (("w2", REPS2), ("cap", REPS))


def batch_sets(t3, name, size, seeds):
    """The frames of a decoded batch: three contents (salt 0, 1, 2) per seed -> [the DecFrames of salt 0, of salt 1, of salt 2]"""
    return [dec_frames(t3, name, size, seeds, salt) for salt in (0, 1, 2)]


def batch_streams(frs):
    """What the batch cells decode of one seed's three frames: frame 0 with t errors at body symbols 0, 1, .., frame 1 with the far
    block, frame 2 with t errors right behind symbols 0 and 1."""
    return [fe.u8(frs[0].le_t()), fe.u8(frs[1].far()), fe.u8(frs[2].tight())]


# ---- what the plans must say ---------------------------------------------------------------------------------------------------------
# Written down here, not read from the library: a FIXED 1-D frame of one k without a beacon is what the fused pixel kernel takes with a
# tile range (window decode) and what a batch runs in one launch (t3_dec_plan.cpp: plan_window, t3_api_encode.cpp: plan_frames).
# tests/test_scrambler_sequences.py::test_plans holds the library's planners against it for every framing, size and class.
TILE_RANGE = {name: int(name in rp.ONE_K) for name in ENC_FRAMINGS}


def windows_of(n):
    """The frame of n pixels read as rows of 64: (label, (fw, fh, x0, y0, w, h)) -- the whole frame as one row, the rows that hold its
    last 200 pixels (a tile range that starts behind tile 0 where the path decodes a range), its first two rows (tile 0)."""
    fh = -(-n // 64); y0 = max(n - 200, 0) // 64
    return (("whole", (n, 1, 0, 0, n, 1)), ("last", (64, fh, 0, y0, 64, fh - y0)), ("first", (64, fh, 0, 0, 64, min(2, fh))))


def batch_encode_one_launch(name, mode, size, front_end):
    """Does a batch encode run as one launch of the batch kernel?  Pixel and RGB input of the tile-range framings; set down for FIXED at
    every size and for COMPAT from the size `tile` on (None: not set down -- a COMPAT frame of one or two words)."""
    if mode == 0 and size in ("w1", "w2") and TILE_RANGE[name] and front_end != "words":
        return None
    return int(bool(TILE_RANGE[name]) and front_end != "words")


def starts_behind_tile0(name, size, label):
    """Does the window's launch start at a tile >= 1?  Only a tile-range framing's, for the last rows of a frame of several tiles."""
    return bool(TILE_RANGE[name]) and size == "cap" and label == "last"


def far_verdict(name, size, label):
    """The far block is block 0 of band 0, in tile 0: a launch over a tile range that starts behind it does not meet it."""
    return [0, 0] if starts_behind_tile0(name, size, label) else [0, 1]


# ---- the image front end -------------------------------------------------------------------------------------------------------------
IMG_SUB, IMG_SRC, IMG_KW = 15, (100, 75), dict(profile=2, uep=2)        # S15, not centred: frames of 854 x 480, the smallest geometry


class ImageCase:
    """Three RGB sources of 100 x 75 and the frames (resize to 854 x 480) the image front end makes of them; per seed the oracle's coded
    frames, and those frames damaged: t errors at body symbols 0, 1, 2 of frame 0, at 2, 3, 4 of frame 2, frame 1's first block replaced by a far row."""

    def __init__(self, t3):
        from test_gpu_window import compose_np
        orc = ol.oracle()
        sw, sh = IMG_SRC
        self.t3 = t3
        self.srcs = [orc.lcg_rgb(sw * sh, 80 + f).reshape(sh, sw, 3) for f in range(3)]
        self.px = [orc.rgb_to_quant(np.ascontiguousarray(compose_np(orc, src, IMG_SUB, False)[0]).reshape(-1)) for src in self.srcs]
        self.n_raw = len(self.px[0]) // 2
        self.rgb = [orc.quant_to_rgb(p) for p in self.px]
        self._coded = {}

    def _one(self, key):
        seed, f = key
        rc, s = ol.oracle().encode_frame(self.px[f], ol.make_cfg(mode=1, **dict(IMG_KW, seed=seed)))
        assert rc == 0
        return _frozen(s)

    def prefetch(self, seeds):
        """The oracle's streams of all three frames under every seed, in one pass of the pool."""
        todo = [(tuple(s), f) for s in seeds for f in range(3) if (tuple(s), f) not in self._coded]
        for k, c in zip(todo, _pool(self._one, todo)):
            self._coded[k] = c

    def coded(self, seed, frames=(0, 1, 2)):
        """The oracle's coded frames under a seed (flat bytes)"""
        keys = [(tuple(seed), f) for f in frames]
        todo = [k for k in keys if k not in self._coded]
        for k, s in zip(todo, _pool(self._one, todo)):
            self._coded[k] = s
        return [self._coded[k] for k in keys]

    def damaged(self, seed, frames=(0, 1, 2)):
        orc = ol.oracle(); ocfg = ol.make_cfg(mode=1, **dict(IMG_KW, seed=tuple(seed)))
        L = self.t3.plan(self.n_raw, self.t3.make_cfg(mode=1, **dict(IMG_KW, seed=tuple(seed))))
        out = []
        for f, c in zip(frames, self.coded(seed, frames)):
            e = [np.zeros((int(L.band_blocks[b]), 26), np.uint8) for b in range(9)]
            e[0][0] = rp.beyond_t(20)["s0"][class_of(seed)] if f == 1 else rp.forced_first(20, f)
            if f == 2:
                e[0][0] = 0; e[0][0][2:5] = (5, 17, 26)                       # none at body symbols 0 and 1, as DecFrame.tight
            out.append(fe.u8(rp.apply(orc, c.reshape(-1, 9), L, ocfg, e)))
        return out


@functools.lru_cache(maxsize=1)
def _image_case(t3):
    return ImageCase(t3)


def image_case(t3):
    return _image_case(t3)
