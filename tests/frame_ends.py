"""Frame sizes at every place a frame can end within a codec tile, and the frames of those sizes (helper module, no tests).

Every codec kernel works tile by tile.  A tile is 9 * Lq stream symbols and Lq is a multiple of the lcm of the band codes the launch
serves (and of 2: t3_enc_plan.cpp takes even multipliers); the decoders' tiles are 9 * nb * k and 9 * lcm * m.  So whatever tile a planner
picks, its boundaries lie on multiples of 9 * lcm(2, subset of the frame's codes).  lattice() brackets every such multiple up to CAP
symbols with raw-word counts W -- built from the codes alone, no planner is asked -- and tests/test_frame_ends_lattice.py proves, against
the library's host-only plans and tests/golden/enc_plan.json, that both sides of every tile step are among them.

A frame of W raw words is n_sym = ceil(26 W / 3) stream symbols; W_le(S) is the largest W whose symbols fit into S.  In FIXED a band's
last block is zero-padded, so the tile count steps right behind W_le(S); in COMPAT the band's tail is dropped and the step comes
9 (k - 1) + 1 symbols later, which is still within a word of a multiple of 9 * lcm(2, k) -- hence the bracket of four words.

Sweep holds the frames of one (configuration, mode): content seeded per (configuration, W), and the CPU oracle's coded stream of every
frame, computed once in a pool of WORKERS threads (the ctypes calls release the GIL) and shared, read-only, by every test of a module."""
import functools
import itertools
import zlib
from concurrent.futures import ThreadPoolExecutor
from math import gcd

import numpy as np

import oracle_lib as ol
import rs_patterns as rp

CAP = 40000                      # symbols: >= 3 tiles of every matrix-core kernel in enc_plan.json (largest 12096) and of the fused decoder
                                 # (largest 9 * 52 * 24 = 11232), one boundary of the largest LUT tile (29808)
DENSE = 130                      # every W in 0 .. DENSE: less than one block per band, bands without a block in COMPAT, the empty frame
BRACKET = (-2, 1)                # W_le(S) - 2 .. W_le(S) + 1 around every boundary S
BEACON_RUN = 120                 # consecutive W whose body ends before, at and behind a beacon slot
EXTRA_MAX = 64                   # at most about this many multiples of a 2-D unit (a row of 1 or 7 symbols has 40000 of them)
WORKERS = 8                      # threads of the oracle pool; a fixed number, not the machine's CPU count
WILD_EVERY = 5                   # every fifth frame holds values outside the codec's range


def lcm(*xs):
    out = 1
    for x in xs:
        out = out * x // gcd(out, x)
    return out


def w_le(S):
    """The largest W with ceil(26 W / 3) <= S."""
    return 3 * S // 26


def n_sym(W):
    return -(-26 * W // 3)


def band_codes(kw):
    """The k of each of the nine bands of a configuration of rs_patterns.CONFIGS / test_gpu_parity.CFGS."""
    uep = kw["uep"]
    bp = [2 if b % 3 == 0 else 1 for b in range(9)] if uep == "luma" else [uep % 4] * 9 if isinstance(uep, int) else list(uep)
    return [rp.K_OF_UEP[p] for p in bp]


def subset_units(ks):
    """9 * lcm(2, subset) for every non-empty subset of the distinct codes."""
    ks = sorted(set(ks))
    return sorted({9 * lcm(2, *sub) for r in range(1, len(ks) + 1) for sub in itertools.combinations(ks, r)})


def _thinned(n):
    """Multipliers 1 .. n of a 2-D unit: all of them up to EXTRA_MAX, else the first three and every ceil(n / EXTRA_MAX)-th."""
    if n <= EXTRA_MAX:
        return range(1, n + 1)
    step = -(-n // EXTRA_MAX)
    return sorted(set(range(1, 4)) | set(range(step, n + 1, step)))


def boundaries(ks, extra_units=()):
    """Every symbol count S <= CAP a tile (or, with extra_units, a 2-D row or interleave chunk) can end at."""
    S = set()
    for u in subset_units(ks):
        S.update(range(u, CAP + 1, u))
    for u in extra_units:
        if u > 0:
            S.update(u * j for j in _thinned(CAP // u))
    return sorted(S)


def lattice(ks, extra_units=(), beacon=False, bracket=BRACKET):
    """Sorted raw-word counts W: the dense run, the bracket around every boundary, and for a beaconed framing one run of BEACON_RUN
    consecutive counts from W_le(three tiles of the frame's lcm) on."""
    W = set(range(DENSE + 1))
    for S in boundaries(ks, extra_units):
        W.update(range(max(w_le(S) + bracket[0], 0), w_le(S) + bracket[1] + 1))
    if beacon:
        w0 = w_le(3 * 9 * lcm(2, *set(ks)))
        W.update(range(w0, w0 + BEACON_RUN))
    return sorted(W)


def lattice_of(kw):
    """The lattice of a configuration given as the keywords of make_cfg."""
    tw, th = kw.get("tile", (0, 0))
    extra = (tw, tw * th) if kw["profile"] == 4 and tw and th else ()
    return lattice(band_codes(kw), extra, bool(kw.get("beacon", (0, 0, 0))[2]))


def pixel_count(W, i):
    """Lattice entry i of W raw words: 2 W pixels, or one less (a pad pixel) at every odd entry."""
    return max(2 * W - (i % 2), 0)


def u8(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


def _frozen(a):
    a = u8(a).copy()
    a.setflags(write=False)
    return a


class Sweep:
    """The frames of one configuration in one mode, one per lattice size.  salt = 0: the sweep proper, whose every fifth frame is out of
    range for the pixel and the raw-word front end (pixel components over the whole of uint16 / int16, word bytes 0 .. 255: the
    expectation is the oracle's, as for any other frame; RGB input is always valid).  salt > 0: further in-range frames of the same
    sizes, for batches.  seed = (a, b, s0): the scrambler seed of every stream (the content does not depend on it).

      case(fe, i)  -> (input bytes, units, the oracle's coded bytes) for fe in "pixels", "rgb", "words"
      px[i]        the in-range pixels of frame i (= rgb_to_quant of its RGB input): what a FIXED decode of stream("rgb", i) gives back"""

    def __init__(self, name, kw, mode, salt=0, seed=(1, 1, 1)):
        self.name, self.kw, self.mode, self.salt = name, dict(kw, seed=tuple(seed)), mode, salt
        self.ocfg = ol.make_cfg(mode=mode, **self.kw)
        self.Ws = lattice_of(kw)
        self.n_px = [pixel_count(W, i) for i, W in enumerate(self.Ws)]
        self._in, self._out = {}, {}
        self.px = None

    def __len__(self):
        return len(self.Ws)

    def wild(self, i):
        return self.salt == 0 and i % WILD_EVERY == WILD_EVERY - 1

    def _rng(self, i, what):
        return np.random.default_rng([zlib.crc32(self.name.encode()), self.Ws[i], self.salt, what])

    def _rgb(self, i):
        orc = ol.oracle()
        rng = self._rng(i, 0)
        rgb = rng.integers(0, 256, 3 * self.n_px[i], dtype=np.uint8)
        snap = rng.integers(0, 4, len(rgb)) == 0                             # a quarter of the components at 0 or 255: saturated colours
        rgb[snap] = 255 * rng.integers(0, 2, int(snap.sum()), dtype=np.uint8)
        px = orc.rgb_to_quant(rgb)
        rc, s = orc.encode_frame(px, self.ocfg, cap=self.n_px[i] + 64)
        assert rc == 0, (self.name, self.mode, self.Ws[i])
        return _frozen(rgb), px, _frozen(s)

    def _wild_px(self, i):
        orc = ol.oracle(); n = self.n_px[i]; rng = self._rng(i, 1)
        px = np.zeros(n, ol.PIXEL_DT)
        px["Yq"] = rng.integers(0, 65536, n); px["Cbq"] = rng.integers(-32768, 32768, n); px["Crq"] = rng.integers(-32768, 32768, n)
        rc, s = orc.encode_frame(px, self.ocfg, cap=n + 64)
        assert rc == 0, (self.name, self.mode, self.Ws[i])
        return _frozen(px), _frozen(s)

    def _words(self, i):
        orc = ol.oracle()
        raw = self._rng(i, 2).integers(0, 256 if self.wild(i) else 27, (self.Ws[i], 9), dtype=np.uint8)
        rc, s = orc.encode_profile(raw, self.ocfg)
        assert rc == 0, (self.name, self.mode, self.Ws[i])
        return _frozen(raw), _frozen(s)

    def _pool(self, fn, idx):
        idx = list(idx)
        if not idx:
            return []
        first = fn(idx[0])                                                   # (the oracle builds its tables on first use)
        with ThreadPoolExecutor(WORKERS) as ex:
            return [first] + list(ex.map(fn, idx[1:]))

    def _ensure(self, fe):
        if fe in self._in:
            return
        n = len(self)
        if fe == "rgb":
            res = self._pool(self._rgb, range(n))
            self._in[fe] = [r[0] for r in res]; self._out[fe] = [r[2] for r in res]
            self.px = [r[1] for r in res]
            for p in self.px:
                p.setflags(write=False)
        elif fe == "pixels":
            self._ensure("rgb")
            ins = [u8(p) for p in self.px]; outs = list(self._out["rgb"])
            wild = [i for i in range(n) if self.wild(i)]
            for i, (p, s) in zip(wild, self._pool(self._wild_px, wild)):
                ins[i], outs[i] = p, s
            self._in[fe], self._out[fe] = ins, outs
        elif fe == "words":
            res = self._pool(self._words, range(n))
            self._in[fe] = [r[0] for r in res]; self._out[fe] = [r[1] for r in res]
        else:
            raise ValueError(fe)

    def units(self, fe, i):
        return self.Ws[i] if fe == "words" else self.n_px[i]

    def case(self, fe, i):
        self._ensure(fe)
        return self._in[fe][i], self.units(fe, i), self._out[fe][i]

    def stream(self, fe, i):
        self._ensure(fe)
        return self._out[fe][i]


@functools.lru_cache(maxsize=4)
def _sweep(name, kw_items, mode, salt):
    return Sweep(name, dict(kw_items), mode, salt)


def sweep(name, kw, mode, salt=0):
    """The shared Sweep of (configuration, mode, salt); a few are kept, so tests run configuration by configuration."""
    return _sweep(name, tuple(sorted((k, tuple(v) if isinstance(v, list) else v) for k, v in kw.items())), mode, salt)
