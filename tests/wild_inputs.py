"""Frames whose out-of-range input values stand ALONE, and frames that hold every input value (helper module, no tests).

Every encoder front end converts its input on a fast path that assumes quantised pixels with Yq in 0 .. 242 and Cbq, Crq in -40 .. 40, or
raw-word bytes 0 .. 26.  The reference clamps nothing: a component counts as its uint32 cast mod 3^w, a word byte mod 27.  So each
converter of csrc/t3_enc_convert.h carries a second, exact reduction behind a wave-uniform ballot ("does any lane of this wave see a wild
value?").  A frame that is wild all over fires every wave's ballot, and the fast path never meets a wild value; a check that misses one
component, one half of a packed register, one byte, or masks a live half away would pass such a frame bit for bit.  Here a wild value is
the only one its wave sees.

P = 769, the distance between the wild values of a frame, read from the converters (one ballot covers one loop step of one wave):
  convert_pixels_packed   a lane takes four consecutive pixel triples, a wave 64 consecutive lane units: 64 * 4 * 3 = 768 consecutive pixels
                          (its two ballots -- triples 0, 2 and triples 1, 3 of every lane -- each cover half of them)
  convert_words_half      a lane unit is four word triples, a wave takes one half (two triples) of 64 consecutive units: 6 of every 12 words
                          of 64 * 12 = 768 consecutive words; the 56 bytes it tests hold two bytes of the neighbouring half
  convert_groups          a lane takes a group of two triples, a ballot one triple of each of 64 consecutive groups: within 64 * 6 = 384 units
  RAW packer              (t3_kernels.hip) reduces every component and byte, no ballot
So 768 consecutive units is the longest run a ballot covers, and two values 769 units apart never share one: in 1-D and in the 2-D flows
that stage whole rows, where a wave's lane units are consecutive.  (The run-placed 2-D flow converts up to three runs of a tile in one
loop; a wave that straddles two runs spans the gap between them and may see two wild values.  The thinned sweeps run there; every unit
is still wild once, and nearly every wave sees one value alone.)

Lone sweep: frame s (s = 0 .. P - 1) of sweep c is the base frame -- in-range random content, the same for all -- with one wild value at every
unit s + j P.  Pixels, c = 0, 1, 2: the component (c + j) % 3 of that pixel; raw words, c = 0 .. 8: byte (w + c) % 9 of word w.  Over the
3 P pixel frames every (pixel, component) is wild exactly once, over the 9 P word frames every (word, byte).  (Lane units start at
multiples of twelve words; sweeps 0, 1, 2 alone reach each of the 12 x 9 byte slots of a unit somewhere -- a word's slot and its byte are
tied mod 3 -- and all nine reach them in every unit.)  That covers every slot of a lane unit (low and high half of the packed registers),
every lane, the first and last unit of every tile and each number of live triples in a tile's last unit by construction: no planner is
asked where a tile ends.

The wild values cycle, with the lane unit u // 12 of the wild unit u = s + j P and with j, through lists that hold both sides of every edge
(the lattice test proves what each one is next to): over the full sweeps every listed value meets each of the 12 x 3 component slots and
each of the 12 x 9 byte slots of a lane unit, and the values of one frame differ.

Base sizes: W_BASE = 3501 raw words = 7001 pixels (an odd count: a pad pixel) = 30342 stream symbols holds two tile boundaries and a
ragged end of every tile the matrix-core kernels take (tests/golden/enc_plan.json: at most 12096 symbols) and of the 704-thread table
kernel (14256), and one boundary of every recorded tile; W_BIG = 6901 words = 13801 pixels = 59809 symbols holds two tiles of the largest
recorded table-kernel tile (29808 symbols) and a ragged end.

Exhaustive frames are dense on purpose: every Yq 0 .. 65535, every Cbq and every Crq -32768 .. 32767, each run three times -- a run of 65536
starts one pixel slot of a triple further each time -- and every byte value at every one of the 108 byte slots of a lane unit of raw
words.  They pin red_y, red_c and mod27 on the device over their whole domain.

The oracle's streams are computed once per (configuration, mode, front end) in a pool of WORKERS threads and shared, read-only."""
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import oracle_lib as ol

P = 769
WORKERS = 8                                       # threads of the oracle pool; a fixed number, not the machine's CPU count
W_BASE, W_BIG = 3501, 6901                        # raw words of the base frames; pixels: 2 W - 1
Y_WILD = (243, 244, 485, 486, 32768, 65535)
C_WILD = (41, 42, -41, -42, 121, 122, 32767, -32768)
B_WILD = (27, 127, 128, 154, 155, 255)
COMPONENTS = ("Yq", "Cbq", "Crq")
PIXEL_SWEEPS, WORD_SWEEPS = (0, 1, 2), tuple(range(9))


def n_px_of(W):
    return 2 * W - 1


def u8(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


def rand_pixels(rng, n):
    px = np.zeros(n, ol.PIXEL_DT)
    px["Yq"] = rng.integers(0, 243, n); px["Cbq"] = rng.integers(-40, 41, n); px["Crq"] = rng.integers(-40, 41, n)
    return px


@functools.lru_cache(maxsize=None)
def base_pixels(W):
    px = rand_pixels(np.random.default_rng([20261, W]), n_px_of(W))
    px.setflags(write=False)
    return px


@functools.lru_cache(maxsize=None)
def base_words(W):
    raw = np.random.default_rng([20262, W]).integers(0, 27, (W, 9), dtype=np.uint8)
    raw.setflags(write=False)
    return raw


LANE_UNIT = 12                                    # pixels / words of a lane's work unit: four triples, units start at multiples of 12


def sites(n_units, s):
    """Frame s: the wild units s + j P of a frame of n_units -> (unit index, j, position in the value cycle).  The position advances with
    the lane unit (at // 12) and with j: P is 1 mod 12, mod 6 and mod 8, so a position of j + s would tie a value to two or three of the
    twelve slots of a lane unit; with at // 12 in it every value meets every slot (the lattice test counts them)."""
    at = np.arange(s, n_units, P)
    j = np.arange(len(at))
    return at, j, at // LANE_UNIT + j


def pixel_sites(n_px, c, s):
    """-> (pixel, component 0 .. 2, position in the value cycle), one entry per wild value of frame s of sweep c"""
    at, j, cyc = sites(n_px, s)
    return at, (c + j) % 3, cyc


def word_sites(W, c, s):
    """-> (word, byte 0 .. 8, position in the value cycle)"""
    at, j, cyc = sites(W, s)
    return at, (at + c) % 9, cyc


def wild_pixel_value(comp, cyc):
    return Y_WILD[cyc % len(Y_WILD)] if comp == 0 else C_WILD[cyc % len(C_WILD)]


def wild_byte_value(cyc):
    return B_WILD[cyc % len(B_WILD)]


def pixel_frame(W, c, s, change=None):
    """Frame s of sweep c.  change: what is planted instead of each wild value (the planted failures of the lattice test)."""
    px = base_pixels(W).copy()
    for at, comp, cyc in zip(*pixel_sites(len(px), c, s)):
        v = wild_pixel_value(int(comp), int(cyc))
        if change is not None:
            v = change(int(comp), v)
        px[COMPONENTS[comp]][at] = v & 0xFFFF if comp == 0 else np.array(v).astype(np.int16)
    return px


def word_frame(W, c, s, change=None):
    raw = base_words(W).copy()
    for at, b, cyc in zip(*word_sites(W, c, s)):
        v = wild_byte_value(int(cyc))
        raw[at, b] = v if change is None else change(v)
    return raw


def clamp_pixel(comp, v):
    """The nearest in-range value."""
    return min(v, 242) if comp == 0 else max(-40, min(v, 40))


def low_byte_pixel(comp, v):
    """The value mod 256: what a conversion sees that drops the upper byte."""
    return v & 0xFF


def clamp_byte(v):
    return min(v, 26)


def pool(fn, items):
    items = list(items)
    if not items:
        return []
    first = fn(items[0])                                                     # (the oracle builds its tables on first use)
    with ThreadPoolExecutor(WORKERS) as ex:
        return [first] + list(ex.map(fn, items[1:]))


def encode(front_end, data, ocfg):
    """The oracle's coded stream of one frame, as bytes."""
    orc = ol.oracle()
    rc, s = orc.encode_frame(data, ocfg) if front_end == "pixels" else orc.encode_profile(data, ocfg)
    assert rc == 0, (front_end, rc)
    return u8(s).copy()


class Sweep:
    """The frames of the component sweeps `cs` of one front end ("pixels" or "words") over the base frame of W words, and the oracle's
    stream of each under one configuration: frame f = (c, s) in the order of cs, s = 0 .. P - 1.
      inputs    (frames, bytes of one frame) uint8      want   (frames, bytes of one stream) uint8      both read-only"""

    def __init__(self, front_end, kw, mode, W, cs):
        self.front_end, self.kw, self.mode, self.W, self.cs = front_end, dict(kw), mode, W, tuple(cs)
        self.ocfg = ol.make_cfg(mode=mode, **self.kw)
        self.index = [(c, s) for c in self.cs for s in range(P)]
        self.n_units = n_px_of(W) if front_end == "pixels" else W
        make = pixel_frame if front_end == "pixels" else word_frame
        self.inputs = np.stack([u8(make(W, c, s)) for c, s in self.index])
        self.want = np.stack(pool(lambda b: encode(front_end, self.frame_of(b), self.ocfg), list(self.inputs)))
        self.inputs.setflags(write=False); self.want.setflags(write=False)

    def __len__(self):
        return len(self.index)

    def frame_of(self, b):
        """A frame's bytes as the oracle takes them: pixel records or (W, 9) words."""
        return b.view(ol.PIXEL_DT) if self.front_end == "pixels" else b.reshape(-1, 9)


@functools.lru_cache(maxsize=2)
def _sweep(front_end, kw_items, mode, W, cs):
    return Sweep(front_end, dict(kw_items), mode, W, cs)


def sweep(front_end, kw, mode, W=W_BASE, cs=PIXEL_SWEEPS):
    """The shared Sweep; two are kept, so tests run configuration by configuration.  cs = (0,): the thinned sweep."""
    return _sweep(front_end, tuple(sorted((k, tuple(v) if isinstance(v, list) else v) for k, v in kw.items())), mode, W, tuple(cs))


# ---- the thinned sweeps' configurations ---------------------------------------------------------------------------------------------------
K20 = dict(profile=2, uep=2)
# name -> (keywords of make_cfg, mode, base words, launches for pixels, launches for raw words); a launch: (kernel kind, threads, il_on,
# il_async) as plan_encode dispatches it -- tests/test_wild_inputs_lattice.py holds the planner to it, so that the conversion path
# tests/test_gpu_wild_inputs.py names for a configuration stays the one it runs
THINNED = {
    "k20_compat": (K20, 0, W_BASE, [("MfmaK", 512, 0, 0)], [("MfmaK", 512, 0, 0)]),
    "luma": (dict(profile=1, uep="luma"), 1, W_BASE, [("Uep", 512, 0, 0)], [("Uep", 512, 0, 0)]),
    "four_codes": (dict(profile=1, uep=[0, 1, 2, 3, 0, 1, 2, 3, 1]), 1, W_BIG, [("Uep", 512, 0, 0)] * 2, [("Uep", 512, 0, 0)] * 2),
    "k20_beacon83": (dict(profile=2, uep=2, beacon=(83, 2, 1)), 1, W_BASE, [("MfmaK", 512, 0, 0)], [("MfmaK", 512, 0, 0)]),
    "2d_64x64_luma": (dict(profile=4, uep="luma", tile=(64, 64)), 1, W_BASE, [("Uep", 512, 1, 1)], [("Uep", 512, 1, 0)]),
    "2d_1024x16_k20": (dict(profile=4, uep=2, tile=(1024, 16)), 1, W_BASE, [("MfmaK", 448, 1, 2)], [("MfmaK", 512, 1, 0)]),
    "2d_513x8_k20": (dict(profile=4, uep=2, tile=(513, 8)), 1, W_BASE, [("MfmaK", 448, 1, 2)], [("MfmaK", 512, 1, 0)]),
    "2d_7x5_k22": (dict(profile=4, uep=1, tile=(7, 5)), 1, W_BASE, [("MfmaK", 448, 1, 1)], [("MfmaK", 512, 1, 0)]),
    "2d_512x8_three_codes": (dict(profile=4, uep=[3, 3, 3, 1, 1, 1, 0, 0, 0], tile=(512, 8)), 1, W_BIG, [("Lut", 704, 1, 1)], [("Uep", 512, 1, 0)]),
}


# ---- exhaustive frames ---------------------------------------------------------------------------------------------------------------------
RUN = 65536
ROTATIONS = 3                                     # 65536 = 1 mod 3: run r of a component starts in pixel slot r of its triple


@functools.lru_cache(maxsize=None)
def exhaustive_pixels():
    """9 runs of 65536 pixels -- Yq, then Cbq, then Crq through its whole domain, three times each, the other two components in range and
    random -- and one more pixel (an odd count)."""
    n = 3 * ROTATIONS * RUN + 1
    px = rand_pixels(np.random.default_rng(20263), n)
    for comp in range(3):
        for r in range(ROTATIONS):
            lo = (ROTATIONS * comp + r) * RUN
            px[COMPONENTS[comp]][lo: lo + RUN] = np.arange(RUN).astype(np.uint16) if comp == 0 else np.arange(-32768, 32768).astype(np.int16)
    px.setflags(write=False)
    return px


@functools.lru_cache(maxsize=None)
def exhaustive_words():
    """1024 word triples: byte p (0 .. 26) of triple 4 u + q is (u + 64 q + 37 p) mod 256, so every byte slot of a lane unit of four triples
    meets every value as u runs through 0 .. 255; and one canonical word more (an odd count)."""
    t = np.arange(1024)[:, None]; p = np.arange(27)[None, :]
    raw = np.zeros((3073, 9), np.uint8)
    raw[:3072] = ((t // 4 + 64 * (t % 4) + 37 * p) % 256).astype(np.uint8).reshape(3072, 9)
    raw[3072] = np.arange(9) + 18
    raw.setflags(write=False)
    return raw


def reduced_components(px):
    """The reference's view of a pixel record, as closed forms in 64-bit integers: Yq % 243, ((Cq + 40) mod 2^32) % 81 -> (n, 3) int64"""
    y = px["Yq"].astype(np.int64) % 243
    cb = ((px["Cbq"].astype(np.int64) + 40) % (1 << 32)) % 81
    cr = ((px["Crq"].astype(np.int64) + 40) % (1 << 32)) % 81
    return np.stack([y, cb, cr], axis=1)


def words_of_components(comps):
    """(n, 3) reduced components -> the packed raw words (ceil(n / 2), 9): a pixel is the 13-trit number Y + 243 (Cb + 81 Cr), a word two of
    them (trit 26 is zero; the pad pixel of an odd count is Y = 0, Cb + 40 = Cr + 40 = 40), a byte three trits, lowest first."""
    v = comps[:, 0] + 243 * (comps[:, 1] + 81 * comps[:, 2])
    if len(v) % 2:
        v = np.append(v, 243 * (40 + 81 * 40))
    w = v[0::2] + 3 ** 13 * v[1::2]
    return np.stack([(w // 27 ** i) % 27 for i in range(9)], axis=1).astype(np.uint8)
