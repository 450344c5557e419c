"""Frame sizes at every place a FIXED frame can end within a tile of an in-place repair, and received streams aimed at that end (helper
module, no tests).

The four repair families (t3_repair.hip, t3_repair_frames.hip, t3_repair_era.hip, t3_repair_era_frames.hip) store into their own
input: all 26 wire positions of an accepted block -- the zero-padded last block of a band included --, the encoder's symbol into
every beacon slot, zero into the up to 8 bytes behind the body (a beacon slot among them left to the beacon loop).  What lies next
to those stores must not change: a refused block, the header of the next frame of a batch, the gap of a stride.

repair_lattice(name)   raw-word counts from the codes and the layout alone (no repair planner is asked): frame_ends' dense run, both
                       sides of every tile boundary up to one fused tile plus two block rows, the bracket around the first three
                       steps of a launch's tile count (fused: 9 * 52 * k symbols; generic: 256 blocks), and for a beaconed framing
                       frame_ends' beacon run plus the first frames whose tail holds a beacon slot.
                       tests/test_repair_ends_lattice.py proves against t3hip_repair_plan that the steps are in it.
end_damage(orc, fr, i) the received stream of a frame: per band the LAST block and block 0 carry an (erased, wrong) kind of
                       erasure_patterns, the second-last a weight-t row -- no more, since the yardstick of the erasure repair
                       tests subsets of positions on every flagged block and is the cost of a sweep --; every tail byte is dirty,
                       canonical (1..26) and above 26 in turn; every beacon slot holds a seeded byte; every 7th frame ends in a
                       refused block.
cases(name, salt)      per lattice size the frame, the stream and both yardsticks' answers (test_repair_semantics.expected, which
                       reads bytes mod 27, and erasure_patterns.expected_erasures: one received stream serves both families),
                       computed once, read-only; plain_cases(name, salt) is the same without the erasure answers, which are most
                       of the work.  One after the other: the yardsticks are many small numpy calls that hold the interpreter
                       lock, and a pool of frame_ends.WORKERS threads took 33 s for the 236 k20 frames that one thread then
                       prepared in 6 s (profiles/repair_ends/notes.md)."""
import collections
import functools
import zlib

import numpy as np

import erasure_patterns as ep
import frame_ends as fe
import oracle_lib as ol
import rs_patterns as rp
from test_repair_semantics import FUSED, expected

ROWS = 54                        # boundaries up to 9 * ROWS * k_max symbols: one fused tile (52 block rows) plus two rows
FUSED_ROWS = 52                  # block rows of a fused tile: 9 * 52 blocks
GENERIC_BLOCKS = 256             # blocks of a workgroup of the generic kernels
STEPS = 3                        # tile-count steps that get the bracket W - 2 .. W + 1
STEP_BRACKET = (-2, 1)
SLOT_FRAMES = 3                  # frames with a beacon slot in the tail, each with both neighbours
FAR_EVERY = 7                    # every 7th frame: a refused block right in front of the tail
CONTENT_SEED = 400               # + salt: the seed of a frame's pixels
LIGHT_SALTS = (1, 2)             # the further frames of a batch: block 0 carries a <= t schedule row, not a kind (half the yardstick's work)

Case = collections.namedtuple("Case", "i W fr rec plain plain_words era era_words far")


def _t3():
    import __graft_entry__ as ge
    return ge.load_package()


def _crc(name):
    return zlib.crc32(name.encode())


def planner(name):
    """(n_raw -> layout, the library's configuration) of a configuration of rs_patterns.CONFIGS in FIXED mode"""
    t3 = _t3()
    cfg = t3.make_cfg(mode=1, **rp.CONFIGS[name])
    return (lambda n_raw: t3.plan(n_raw, cfg)), cfg


def make_frame(orc, name, W, i, salt=0):
    """Lattice entry i of W raw words: frame_ends.pixel_count pixels (the pad pixel alternates), content by (salt, size)"""
    return rp.Frame(orc, planner(name)[0], name, fe.pixel_count(W, i), CONTENT_SEED + salt)


# ---- where the tail holds a beacon slot ----------------------------------------------------------------------------------------------
def tail_parts(L, ocfg):
    """-> (flat indices of the tail bytes that are no beacon slot, flat indices of the beacon slots at or behind the body's end)"""
    B = rp.block_index(L, ocfg); at = rp.beacon_index(L, ocfg)
    end = int(B.max()) + 1 if B.size else int(L.header_syms)
    tail = np.arange(end, 9 * int(L.out_words), dtype=np.int64)
    return tail[~np.isin(tail, at)], at[at >= end]


@functools.lru_cache(maxsize=None)
def slot_in_tail(name):
    """The first SLOT_FRAMES raw-word counts up to W_le(CAP) + 1 whose tail holds a beacon slot (none: an empty tuple)"""
    if not rp.CONFIGS[name].get("beacon", (0, 0, 0))[2]:
        return ()
    plan, _ = planner(name); ocfg = ol.make_cfg(mode=1, **rp.CONFIGS[name])
    out = []
    for W in range(1, fe.w_le(fe.CAP) + 2):
        if len(tail_parts(plan(W), ocfg)[1]):
            out.append(W)
            if len(out) == SLOT_FRAMES:
                break
    return tuple(out)


# ---- the sizes ------------------------------------------------------------------------------------------------------------------------
def generic_steps(name, n=STEPS):
    """The first n raw-word counts at which the blocks of all bands -- sum of band_blocks of the layout -- pass a multiple of 256"""
    plan, _ = planner(name)
    out, prev = [], None
    for W in range(1, fe.w_le(fe.CAP) + 2):
        L = plan(W)
        c = -(-sum(int(L.band_blocks[b]) for b in range(9)) // GENERIC_BLOCKS)
        if prev is not None and c != prev:
            out.append(W)
            if len(out) == n:
                break
        prev = c
    return out


def fused_steps(k, n=STEPS):
    """FIXED pads a band's last block, so the tile count steps right behind W_le(9 * 52 * k * j)"""
    return [fe.w_le(9 * FUSED_ROWS * k * j) + 1 for j in range(1, n + 1)]


@functools.lru_cache(maxsize=None)
def repair_lattice(name):
    kw = rp.CONFIGS[name]
    ks = fe.band_codes(kw)
    tw, th = kw.get("tile", (0, 0))
    extra = (tw, tw * th) if kw["profile"] == 4 and tw and th else ()
    beacon = bool(kw.get("beacon", (0, 0, 0))[2])
    W = set(range(1, fe.DENSE + 1))
    for S in fe.boundaries(ks, extra):
        if S <= 9 * ROWS * max(ks):
            W.update((fe.w_le(S), fe.w_le(S) + 1))
    if beacon:                                                               # the run frame_ends.lattice adds
        w0 = fe.w_le(3 * 9 * fe.lcm(2, *set(ks)))
        W.update(range(w0, w0 + fe.BEACON_RUN))
    for s in (fused_steps(ks[0]) if name in FUSED else generic_steps(name)):
        W.update(range(s + STEP_BRACKET[0], s + STEP_BRACKET[1] + 1))
    if beacon:
        have = [w for w in slot_in_tail(name) if w in W]
        for w in slot_in_tail(name):
            if len(have) >= SLOT_FRAMES:
                break
            if w not in have:
                W.update((w - 1, w, w + 1)); have.append(w)
    W.discard(0)
    return tuple(sorted(W))


# ---- the received stream ----------------------------------------------------------------------------------------------------------------
def kinds(k):
    return ep.admissible(k) + ep.beyond(k)


def end_damage(orc, fr, i, salt=0, far=None):
    """-> the received stream of frame `fr`, flat uint8; seeded by (configuration, raw words, i, salt).  Per band b of nb blocks, P =
    kinds(k_b): the last block carries P[(i + 3 b) % |P|], block 0 (nb >= 2) P[(i + 5 b + 7) % |P|], the second-last (nb >= 3) a
    weight-t row of rs_patterns.canonical, of the blocks between every fourth a <= t schedule row; the rest are clean.  far (default:
    every FAR_EVERY-th i): the last block of the last band that holds one carries a row of rs_patterns.far_errors instead.  Every tail
    byte that is no beacon slot is dirty, 1..26 and 27..255 alternating by position and by i; every beacon slot holds a seeded byte,
    the last one a byte that is not the encoder's.  The header stays clean.  salt in LIGHT_SALTS: block 0 carries a schedule row."""
    L = fr.L
    far = (i % FAR_EVERY == FAR_EVERY - 1) if far is None else far
    seed = [_crc(fr.name), fr.n_raw, i, salt]
    B = rp.block_index(L, fr.ocfg)
    clean = fr.clean.reshape(-1)
    last_band = max([b for b in range(9) if fr.blocks[b]], default=-1)
    errs, masks = [], []
    for b in range(9):
        k, nb = fr.ks[b], fr.blocks[b]
        P = kinds(k); t = rp.tparam(k)
        err = np.zeros((nb, 26), np.uint8); mask = np.zeros((nb, 26), bool)
        sched, wt = rp.canonical(k, i % 2)
        at, pairs = [], []
        if nb >= 1:
            at.append(nb - 1); pairs.append(P[(i + 3 * b) % len(P)])
        if nb >= 2 and salt not in LIGHT_SALTS:
            at.append(0); pairs.append(P[(i + 5 * b + 7) % len(P)])
        if at:
            e2, m2 = ep.damage_rows(pairs, seed + [b])
            err[at] = e2; mask[at] = m2
        if nb >= 3:
            full = np.flatnonzero(wt == t)
            err[nb - 2] = sched[full[(i + b) % len(full)]]
        m = np.arange(1, max(nb - 2, 1))
        m = m[m % 4 == 1]
        if nb >= 2 and salt in LIGHT_SALTS:
            m = np.append(m, 0)
        err[m] = sched[(7 * m + b + i) % len(sched)]
        if far and b == last_band:
            pool = rp.far_errors(k)
            err[nb - 1] = pool[(i // FAR_EVERY + 5 * salt) % len(pool)]; mask[nb - 1] = False
        errs.append(err); masks.append(mask)
    flat = rp.apply(orc, fr.clean, L, fr.ocfg, errs).reshape(-1).copy()
    mask = np.concatenate(masks)
    by = ep.ByteSource().fill(clean[B], mask)
    flat[B[mask]] = by[mask]
    rng = np.random.default_rng(seed + [99])
    tail, _ = tail_parts(L, fr.ocfg)
    low = (np.arange(len(tail)) + i + salt) % 2 == 0
    flat[tail] = np.where(low, rng.integers(1, 27, len(tail)), rng.integers(27, 256, len(tail)))
    at = rp.beacon_index(L, fr.ocfg)
    if len(at):
        flat[at] = rng.integers(0, 256, len(at))
        flat[at[-1]] = (int(clean[at[-1]]) + 1 + int(rng.integers(0, 255))) % 256
    return flat


# ---- the cases of a sweep ---------------------------------------------------------------------------------------------------------------
def make_plain(orc, name, W, i, salt=0, far=None):
    """Frame, stream and the plain yardstick's answer: a Case whose era fields are None"""
    fr = make_frame(orc, name, W, i, salt)
    fr.px = fr.padded = None                                                 # (not needed here; a sweep holds hundreds of frames)
    has_far = (i % FAR_EVERY == FAR_EVERY - 1) if far is None else far
    rec = end_damage(orc, fr, i, salt, has_far)
    plain, plain_words, _ = expected(orc, fr, rec)
    for a in (rec, plain, fr.clean):
        a.setflags(write=False)
    return Case(i, W, fr, rec, plain, plain_words, None, None, has_far)


def with_erasures(orc, c):
    """The Case with the erasure yardstick's answer (nine tenths of a sweep's preparation: it tests subsets of positions per flagged block)"""
    era, era_words, _ = ep.expected_erasures(orc, c.fr, c.rec)
    era.setflags(write=False)
    return c._replace(era=era, era_words=era_words)


def make_case(orc, name, W, i, salt=0, far=None):
    return with_erasures(orc, make_plain(orc, name, W, i, salt, far))


# (all sweeps of all salts together: about 2.5 M words, 150 MB; the two yardsticks are cached apart, so that a test of the plain repair
# does not wait for the erasure yardstick)
@functools.lru_cache(maxsize=None)
def plain_cases(name, salt=0):
    """One Case without the erasure answer per entry of repair_lattice(name).  salt = 0: the sweep proper, a far row in every
    FAR_EVERY-th frame.  salt > 0: further frames of the same sizes with other content and other damage, for batches; salt = 1 holds
    the far rows, salt = 2 none."""
    orc = ol.oracle()
    return tuple(make_plain(orc, name, W, i, salt, None if salt < 2 else False) for i, W in enumerate(repair_lattice(name)))


@functools.lru_cache(maxsize=None)
def cases(name, salt=0):
    """plain_cases(name, salt) with the erasure yardstick's answers"""
    orc = ol.oracle()
    return tuple(with_erasures(orc, c) for c in plain_cases(name, salt))
