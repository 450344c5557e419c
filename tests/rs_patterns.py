"""Error patterns for the FIXED (v6c) RS(26, k) decoders, and the yardsticks the tests of those decoders use (helper module, no tests).

Independent part: GF(27) add / sub / mul tables and the syndromes S_j = sum_i c_i alpha^((j+1) i) of a 26-symbol row -- table arithmetic
only, no locator, no Chien search, no Forney.  From them:
  is_codeword    all syndromes zero
  near_table     k = 24, 22: every syndrome vector reachable with <= t errors (27^2 / 27^4 entries; S(c + e) = S(e))
  schedule       the deterministic <= t error patterns a band carries (every single error, every position pair, ...)
  beyond_t       weight t+1 / t+2 patterns split by the CODEWORD criterion (near: a codeword within distance t; far: none), and rows
                 whose syndromes are (s, 0, ..., 0): far for every k, accepted by a decoder that tests #roots = deg sigma only
  block_rows     the received rows of the block-level tests: FIXED codewords plus the schedule, near rows and far rows
  apply          GF(27)-additive error rows onto the coded body of a FIXED stream (with or without beacon)
  lift           received bytes above 26 (congruent mod 27, every value 27..255 at every position, random beacon-slot bytes) on top of those
and the frame builders the CPU proofs (test_fixed_rs_semantics.py, test_noncanonical_semantics.py) and the GPU tests
(test_gpu_fixed_errors.py, test_gpu_noncanonical.py) share."""
import functools
import itertools

import numpy as np

import oracle_lib as ol

K_OF_UEP = {0: 24, 1: 22, 2: 20, 3: 18}
ZEROS = 26                 # clean blocks between the weight-1 and the weight-2 part of the schedule
PER_WEIGHT = 2000          # seeded position sets per weight 3..t (plus the five constructed ones)
POOL_N, POOL_SEED = 200_000, 20261016


def tparam(k):
    return (26 - k) // 2


# ---- the field ---------------------------------------------------------------------------------------------------------------------
class Field:
    """GF(27) from the oracle's exp / mul / inv tables; addition is trit-wise (symbol = t0 + 3 t1 + 9 t2)."""

    def __init__(self, orc):
        t = orc.gf_tables()
        self.exp = t["exp"][:26].astype(np.int64)
        self.mul = t["mul"].reshape(27, 27).astype(np.uint8)
        self.inv = t["inv"].astype(np.uint8)
        a = np.arange(27)
        dig = lambda x, i: (x // 3 ** i) % 3
        self.add = sum(((dig(a[:, None], i) + dig(a[None, :], i)) % 3) * 3 ** i for i in range(3)).astype(np.uint8)
        self.sub = sum(((dig(a[:, None], i) - dig(a[None, :], i)) % 3) * 3 ** i for i in range(3)).astype(np.uint8)

    SMALL = 256                                                               # rows: below it syndromes_small is the faster form

    def syndromes(self, rows, R):
        rows = np.asarray(rows, np.uint8).reshape(-1, 26)
        return self.syndromes_small(rows, R) if len(rows) < self.SMALL else self.syndromes_loop(rows, R)

    def syndromes_small(self, rows, R):
        """The same syndromes in a handful of numpy calls, for the few rows of one block or one band (the yardsticks ask thousands of
        times): all R x 26 products at once, then the field's addition -- trit-wise -- as a sum mod 3 of each trit plane.
        tests/test_repair_ends_lattice.py holds it to syndromes_loop."""
        rows = np.asarray(rows, np.uint8).reshape(-1, 26)
        E = self.exp[(np.arange(1, R + 1)[:, None] * np.arange(26)[None, :]) % 26]                # (R, 26): alpha^((j+1) i)
        terms = self.mul[rows[:, None, :], E[None, :, :]]                                         # (n, R, 26)
        return sum((((terms // 3 ** d) % 3).sum(axis=2, dtype=np.uint16) % 3) * 3 ** d for d in range(3)).astype(np.uint8).reshape(len(rows), R)

    def syndromes_loop(self, rows, R):
        rows = np.asarray(rows, np.uint8).reshape(-1, 26)
        S = np.zeros((len(rows), R), np.uint8)
        for j in range(R):
            acc = np.zeros(len(rows), np.uint8)
            for i in range(26):
                acc = self.add[acc, self.mul[rows[:, i], self.exp[((j + 1) * i) % 26]]]
            S[:, j] = acc
        return S

    def solve(self, A, b):
        """x with A x = b over GF(27), A square and regular (Gaussian elimination)."""
        n = len(b)
        M = np.concatenate([np.asarray(A, np.uint8), np.asarray(b, np.uint8).reshape(n, 1)], axis=1)
        for c in range(n):
            p = c + int(np.flatnonzero(M[c:, c])[0])
            M[[c, p]] = M[[p, c]]
            M[c] = self.mul[self.inv[M[c, c]], M[c]]
            for r in range(n):
                if r != c and M[r, c]:
                    M[r] = self.sub[M[r], self.mul[M[r, c], M[c]]]
        return M[:, n].copy()


_field = None


def field(orc):
    global _field
    if _field is None:
        _field = Field(orc)
    return _field


def is_codeword(orc, k, rows):
    return ~field(orc).syndromes(rows, 26 - k).any(axis=1)


def synd_index(S):
    return (S.astype(np.int64) * (27 ** np.arange(S.shape[1], dtype=np.int64))).sum(axis=1)


@functools.lru_cache(maxsize=None)
def _near_table(k):
    F = field(ol.oracle()); R = 26 - k; t = tparam(k)
    assert t <= 2, "27^R entries: k = 24 and 22 only"
    e = np.zeros((677, 26), np.uint8); i = np.arange(676); e[1 + i, i // 26] = i % 26 + 1      # every pattern of weight <= 1
    S1 = F.syndromes(e, R)
    tab = np.zeros(27 ** R, bool)
    if t == 1:
        tab[synd_index(S1)] = True
    else:                                                                                       # all sums of two of them: weight <= 2
        S2 = F.add[S1[:, None, :], S1[None, :, :]].reshape(-1, R)
        tab[synd_index(S2)] = True
    return tab


def near_by_table(orc, k, rows):
    """k = 24, 22, exact: a codeword lies within distance t of each row <=> its syndrome vector is that of a pattern of weight <= t."""
    return _near_table(k)[synd_index(field(orc).syndromes(rows, 26 - k))]


def sphere_density(k):
    """Share of all 27^26 words within distance t of a codeword: sum_{i <= t} C(26, i) 26^i / 27^R (the spheres are disjoint)."""
    from math import comb
    return sum(comb(26, i) * 26 ** i for i in range(tparam(k) + 1)) / 27 ** (26 - k)


# ---- the <= t schedule ---------------------------------------------------------------------------------------------------------------
def _rows_at(pos_sets, rng):
    e = np.zeros((len(pos_sets), 26), np.uint8)
    for i, ps in enumerate(pos_sets):
        e[i, list(ps)] = rng.integers(1, 27, len(ps))
    return e


def _random_rows(n, w, rng):
    """n error rows of weight w: positions a uniform w-subset, values uniform in 1..26"""
    pos = np.argsort(rng.random((n, 26)), axis=1)[:, :w]
    e = np.zeros((n, 26), np.uint8)
    e[np.arange(n)[:, None], pos] = rng.integers(1, 27, (n, w))
    return e


@functools.lru_cache(maxsize=None)
def canonical(k, seed):
    """The schedule proper, in band order: (rows (n, 26) of additive error values, weight (n,)).  Weight 1 first, then ZEROS clean
    blocks, then weight 2, 3, .. t: from row 676 + ZEROS on every block carries >= 2 errors."""
    t = tparam(k); rng = np.random.default_rng([seed, k])
    i = np.arange(676)
    e1 = np.zeros((676, 26), np.uint8); e1[i, i // 26] = i % 26 + 1                               # every (position, value)
    parts = [e1, np.zeros((ZEROS, 26), np.uint8)]
    if t >= 2:
        parts.append(_rows_at(list(itertools.combinations(range(26), 2)), rng))                   # every position pair
        e2 = np.zeros((676, 26), np.uint8); e2[:, 0] = i // 26 + 1; e2[:, 25] = i % 26 + 1         # every value pair at (0, 25)
        parts.append(e2)
    for w in range(3, t + 1):
        lo = k - (w + 1) // 2                                                                     # a run across k - 1 | k
        built = [rng.choice(k, w, replace=False), k + rng.choice(26 - k, w, replace=False), range(w), range(26 - w, 26), range(lo, lo + w)]
        parts.append(_rows_at(built, rng))
        parts.append(_random_rows(PER_WEIGHT, w, rng))
    rows = np.concatenate(parts)
    rows.setflags(write=False)
    return rows, (rows != 0).sum(axis=1)


def schedule_len(k):
    return len(canonical(k, 0)[0])


def forced_first(k, seed):
    """Block 0: t errors that include positions 0 and 1, the scrambler's two special first symbols (t = 1: one of them, by the seed)."""
    t = tparam(k); rng = np.random.default_rng([seed, k, 1])
    return _rows_at([[seed % 2] if t == 1 else range(t)], rng)[0]


def forced_last(k, seed):
    """A band's last block: t errors, one of them at data position k - 1 (zero padding whenever the block is padded at all)."""
    t = tparam(k); rng = np.random.default_rng([seed, k, 2])
    return _rows_at([[k - 1] + list(range(2, 1 + t))], rng)[0]


def schedule(k, n_blocks, seed):
    """-> (errors (n_blocks, 26), received): block 0 = forced_first, block m >= 1 = canonical row (m - 1) mod its length, the last block =
    forced_last.  received[w] = how many different canonical rows of weight w the band holds."""
    rows, wt = canonical(k, seed)
    e = np.zeros((n_blocks, 26), np.uint8)
    if n_blocks == 0:
        return e, {w: 0 for w in range(tparam(k) + 1)}
    idx = (np.arange(n_blocks) - 1) % len(rows)
    e[:] = rows[idx]
    e[0] = forced_first(k, seed)
    e[-1] = forced_last(k, seed)
    got = np.unique(idx[1:-1])
    return e, {w: int((wt[got] == w).sum()) for w in range(tparam(k) + 1)}


def schedule_totals(k):
    wt = canonical(k, 0)[1]
    return {w: int((wt == w).sum()) for w in range(tparam(k) + 1)}


def assert_coverage(k, received):
    """All of weight 1 and weight 2, >= 500 of each higher weight up to the band's own t."""
    tot = schedule_totals(k)
    for w in range(1, tparam(k) + 1):
        assert received[w] >= (tot[w] if w <= 2 else 500), (k, w, received, tot)


# ---- beyond t ------------------------------------------------------------------------------------------------------------------------
def s0_rows(orc, k, seed=7):
    """52 error rows with syndromes (s, 0, .., 0), s = 1..26: the R x R Vandermonde system V[j][q] = alpha^((j+1) p_q) solved for the error
    values at R positions -- the parity positions, and R seeded positions that include data symbols."""
    F = field(orc); R = 26 - k; rng = np.random.default_rng([seed, k, 3])
    out = []
    for s in range(1, 27):
        mixed = np.sort(np.concatenate([rng.choice(k, R - 1, replace=False), [k + int(rng.integers(0, R))]]))
        for ps in (np.arange(k, 26), mixed):
            V = np.array([[F.exp[((j + 1) * int(p)) % 26] for p in ps] for j in range(R)], np.uint8)
            x = F.solve(V, [s] + [0] * (R - 1))
            e = np.zeros(26, np.uint8); e[ps] = x
            out.append(e)
    out = np.array(out)
    S = F.syndromes(out, R)
    assert (S[:, 0] == np.repeat(np.arange(1, 27), 2)).all() and not S[:, 1:].any()
    return out


@functools.lru_cache(maxsize=None)
def _beyond_t(k, n, seed):
    orc = ol.oracle(); F = field(orc); t = tparam(k)
    rng = np.random.default_rng([seed, k, 4])
    pools = {"t+1": _random_rows(n, t + 1, rng), "t+2": _random_rows(n, t + 2, rng)}
    e = np.concatenate([pools["t+1"], pools["t+2"]])
    if t <= 2:
        near = near_by_table(orc, k, e)
    else:
        # The oracle's verdict on the pattern itself (the zero word is a codeword).  One side is exact here and now: an accepted row came
        # back as a codeword within t symbols.  The other side (no rejected row has one) rests on test_fixed_rs_semantics B1: accepted
        # share of random words = the sphere-packing density.
        cw, _, ok = orc.rs_decode_blocks(k, e, mode=1)
        near = ok == 1
        assert is_codeword(orc, k, cw[near]).all() and ((cw[near] != e[near]).sum(axis=1) <= t).all()
    s0 = s0_rows(orc, k)
    if t <= 2:
        assert not near_by_table(orc, k, s0).any()
    for a in (e, near, s0):
        a.setflags(write=False)
    return {"rows": e, "near": near, "s0": s0, "pools": pools}


def beyond_t(k, n=POOL_N, seed=POOL_SEED, orc=None):
    """-> dict: rows (2 n, 26) error patterns of weight t+1 (first n) and t+2, near (2 n,) bool by the codeword criterion, s0 (52, 26)."""
    return _beyond_t(k, n, seed)


@functools.lru_cache(maxsize=None)
def near_errors(k):
    b = beyond_t(k); a = b["rows"][b["near"]]; a.setflags(write=False); return a


@functools.lru_cache(maxsize=None)
def far_errors(k):
    """(s, 0, .., 0) rows first, then the far rows of the pool (built once per code: Frame.far asks for it per row)"""
    b = beyond_t(k); a = np.concatenate([b["s0"], b["rows"][~b["near"]]]); a.setflags(write=False); return a


# ---- block-level rows ------------------------------------------------------------------------------------------------------------------
BLOCK_POOL = 3000          # near rows and far rows per code the block-level and stage tests take


@functools.lru_cache(maxsize=None)
def block_rows(k):
    """The received rows of the block-level tests (test_rs_block_semantics.py, test_oracle_vs_ref.py, test_gpu_rs_blocks.py):
    -> dict cw (n, 26) FIXED codewords of seeded data, e (n, 26) the whole schedule, then near_errors[:BLOCK_POOL], then
    far_errors[:BLOCK_POOL], rx = cw + e in the field, and the slices sched / near / far into them."""
    orc = ol.oracle(); F = field(orc)
    parts = {"sched": canonical(k, 0)[0], "near": near_errors(k)[:BLOCK_POOL], "far": far_errors(k)[:BLOCK_POOL]}
    e = np.concatenate(list(parts.values()))
    data = np.random.default_rng([20261021, k]).integers(0, 27, size=(len(e), k), dtype=np.uint8)
    cw = orc.rs_encode_blocks(k, data, mode=1)
    out = {"cw": cw, "e": e, "rx": F.add[cw, e]}
    at = 0
    for name, rows in parts.items():
        out[name] = slice(at, at + len(rows)); at += len(rows)
    for a in (out["cw"], out["e"], out["rx"]):
        a.setflags(write=False)
    return out


# ---- streams -------------------------------------------------------------------------------------------------------------------------
def body_index(L, cfg):
    """Flat stream index of every coded body symbol, in body order (with a beacon: the framed positions that are not beacon slots)."""
    hs = int(L.header_syms)
    if not L.beacon_on:
        return hs + np.arange(int(L.body_syms), dtype=np.int64)
    slot, period = int(cfg.beacon_band_slot), int(cfg.beacon_words_period)
    pos = np.arange(int(L.body_syms_framed), dtype=np.int64)
    return hs + np.flatnonzero(~((pos >= slot) & ((pos - slot) % (9 * period) == 0)))[: int(L.body_syms)]


def apply(orc, stream, L, cfg, per_band_errors):
    """stream (n, 9) + per band an (band_blocks, 26) array of additive error values -> the corrupted stream.  The scrambler subtracts a state
    from every trit, so an additive error on the wire is the same additive error on the descrambled block: added in the field."""
    F = field(orc)
    flat = np.ascontiguousarray(stream, np.uint8).reshape(-1).copy()
    bi = body_index(L, cfg)
    for b in range(9):
        e = np.asarray(per_band_errors[b], np.uint8)
        assert e.shape == (int(L.band_blocks[b]), 26)
        at = bi[int(L.band_body_off[b]): int(L.band_body_off[b]) + e.size]
        flat[at] = F.add[flat[at], e.reshape(-1)]
    return flat.reshape(-1, 9)


# ---- frames shared by the CPU proof and the GPU tests ---------------------------------------------------------------------------------
ONE_K = ("k24", "k22", "k20", "k18")
CONFIGS = {
    "k24": dict(profile=0, uep=0), "k22": dict(profile=1, uep=1), "k20": dict(profile=2, uep=2), "k18": dict(profile=3, uep=3),
    "k22_beacon2_slot8": dict(profile=1, uep=1, beacon=(2, 8, 1)), "k20_beacon83": dict(profile=2, uep=2, beacon=(83, 2, 1)),
    "luma": dict(profile=1, uep="luma"), "uep_18_22": dict(profile=1, uep=[3, 1, 1, 3, 1, 1, 3, 1, 1]), "uep_20_24": dict(profile=1, uep=[2, 0, 2, 0, 2, 0, 2, 0, 2]),
    "four_codes": dict(profile=1, uep=[0, 1, 2, 3, 0, 1, 2, 3, 1]),
    "2d_64x64_k20": dict(profile=4, uep=2, tile=(64, 64)), "2d_luma_1024x16": dict(profile=4, uep="luma", tile=(1024, 16)), "2d_7x5_k22": dict(profile=4, uep=1, tile=(7, 5)),
}
SMALL_PX = 301                                    # below one pixel tile (108 k pixels), odd
MIN_BLOCKS_ONE_K = 66 * 52                        # one-k 1-D frames: >= 64 decoder tiles, where the host entry decodes chunk by chunk


def rand_pixels(rng, n):
    px = np.zeros(n, ol.PIXEL_DT)
    px["Yq"] = rng.integers(0, 243, n); px["Cbq"] = rng.integers(-40, 41, n); px["Crq"] = rng.integers(-40, 41, n)
    return px


def frame_sizes(plan, name):
    """Pixel counts for a configuration: 'full' = the smallest even count whose every band holds its schedule once (+ the two forced
    blocks; one k, 1-D: and MIN_BLOCKS_ONE_K blocks), 'padded' = the next odd count at which the last block of every band is
    zero-padded, 'small' = under one tile.  plan(n_raw_words) -> layout."""
    floor = MIN_BLOCKS_ONE_K if name in ONE_K else 0
    def fits(n_px):
        L = plan((n_px + 1) // 2)
        return all(int(L.band_blocks[b]) >= max(schedule_len(int(L.band_k[b])) + 2, floor) for b in range(9))
    lo, hi = 1, 1 << 21
    while lo < hi:
        mid = (lo + hi) // 2
        if fits(2 * mid): hi = mid
        else: lo = mid + 1
    full = 2 * lo
    n = full + 1
    while True:
        L = plan((n + 1) // 2)
        if all(int(L.band_len[b]) % int(L.band_k[b]) for b in range(9)):
            break
        n += 2
    return {"full": full, "padded": n, "small": SMALL_PX}


SIZE_SEED = {"full": 100, "padded": 101, "small": 102}
# the corrupted streams of each size: the <= t schedule, the near-only frame, the frames with M far rows
CASES = {"full": ("sched", "near", "far1", "far2", "far1000"), "padded": ("sched", "far2"), "small": ("sched", "far1")}


def make_frame(orc, plan, name, what, scr=(1, 1, 1)):
    return Frame(orc, plan, name, frame_sizes(plan, name)[what], SIZE_SEED[what], scr)


class Frame:
    """One configuration at one size: pixels, the clean stream (the oracle's encoder, so that both users hold the same bytes), and the
    corrupted streams with what each of them must decode to.  scr = (a, b, s0): the scrambler seed of the stream (`seed` is the
    content's); the default is make_cfg's, and pixels and error patterns do not depend on it."""

    def __init__(self, orc, plan, name, n_px, seed, scr=(1, 1, 1)):
        self.name, self.kw, self.n_px, self.seed = name, dict(CONFIGS[name], seed=tuple(scr)), n_px, seed
        self.ocfg = ol.make_cfg(mode=1, **self.kw)
        self.n_raw = (n_px + 1) // 2
        self.L = L = plan(self.n_raw)
        self.ks = [int(L.band_k[b]) for b in range(9)]
        self.blocks = [int(L.band_blocks[b]) for b in range(9)]
        rng = np.random.default_rng([seed, n_px])
        self.px = rand_pixels(rng, n_px)
        self.padded = np.zeros(2 * self.n_raw, ol.PIXEL_DT); self.padded[:n_px] = self.px
        rc, enc = orc.encode_frame(self.px, self.ocfg, cap=n_px + 64)
        assert rc == 0
        self.clean = np.ascontiguousarray(enc).copy()
        self.orc = orc

    def last_block_padded(self, b):
        return int(self.L.band_len[b]) % self.ks[b] != 0

    def sched_errors(self):
        out, rec = [], []
        for b in range(9):
            e, r = schedule(self.ks[b], self.blocks[b], self.seed)
            out.append(e); rec.append(r)
        return out, rec

    def sched(self):
        """<= t errors everywhere, every band at its own t -> (stream, per-band coverage)"""
        e, rec = self.sched_errors()
        return apply(self.orc, self.clean, self.L, self.ocfg, e), rec

    def near(self, per_code=200):
        """>= per_code near rows per code (never in a band's last block), the rest clean -> (stream, rows placed per code)"""
        rng = np.random.default_rng([self.seed, 5])
        errs = [np.zeros((self.blocks[b], 26), np.uint8) for b in range(9)]
        placed = {}
        for k in sorted(set(self.ks)):
            bands = [b for b in range(9) if self.ks[b] == k and self.blocks[b] > 1]
            pool = near_errors(k)
            want = min(per_code, sum(self.blocks[b] - 1 for b in bands))
            slots = [(b, m) for b in bands for m in range(self.blocks[b] - 1)]
            pick = rng.choice(len(slots), want, replace=False)
            rows = pool[rng.choice(len(pool), want, replace=False)]
            for (b, m), r in zip([slots[i] for i in pick], rows):
                errs[b][m] = r
            placed[k] = want
        return apply(self.orc, self.clean, self.L, self.ocfg, errs), placed

    def far(self, M):
        """The <= t schedule with M blocks replaced by far rows -> (stream, [(band, block)] of the far rows).  M = 1: an (s, 0, .., 0) row in
        block 0 of band 0; M = 2: also the last block of the last band; larger M: also 52 (s, 0, .., 0) rows per code, blocks 52..103 of
        every band (one whole pixel tile of the one-k framing) as far as they exist, and seeded blocks over all bands in the even-numbered
        runs of 52 blocks, so that every other pixel tile of the one-k framing holds no far row."""
        rng = np.random.default_rng([self.seed, 6, M])
        errs, _ = self.sched_errors()
        where = [(0, 0)]
        if M >= 2:
            where.append((8, self.blocks[8] - 1))
        if M > 2:
            free = [(b, m) for b in range(9) for m in range(1, self.blocks[b] - (1 if b == 8 else 0))]
            tile = [(b, m) for (b, m) in free if 52 <= m < 104]
            tile_set = set(tile)
            rest = [s for s in free if s not in tile_set and (s[1] // 52) % 2 == 0]    # odd tiles (but tile 1) stay free of far rows
            where += tile[: M - 2]
            need = M - len(where)
            assert need <= len(rest), "frame too small for %d far rows" % M
            where += [rest[i] for i in rng.choice(len(rest), need, replace=False)]
        assert len(where) == M and len(set(where)) == M
        used = {}
        for (b, m) in where:
            k = self.ks[b]; pool = far_errors(k)
            i = used.get(k, 0); used[k] = i + 1
            # the first 52 rows placed per code are the (s, 0, .., 0) rows, then seeded far rows of the pool
            errs[b][m] = pool[i] if i < 52 else pool[52 + int(rng.integers(0, len(pool) - 52))]
        self.s0_placed = {k: min(n, 52) for k, n in used.items()}
        return apply(self.orc, self.clean, self.L, self.ocfg, errs), where


    def stream(self, case):
        """-> (corrupted stream, M = number of far rows in it, where they are)"""
        if case == "sched":
            return self.sched()[0], 0, []
        if case == "near":
            return self.near()[0], 0, []
        M = int(case[3:])
        s, where = self.far(M)
        return s, M, where


def far_tiles_one_k(k, where):
    """One-k 1-D framing: the pixel tiles (52 blocks of each band, 108 k pixels) that hold a far block."""
    return sorted({m // 52 for (_, m) in where})


def pixels_outside_tiles(n_px, k, tiles):
    keep = np.ones(n_px, bool)
    for t in tiles:
        keep[t * 108 * k: (t + 1) * 108 * k] = False
    return keep


# ---- received bytes 27..255 -----------------------------------------------------------------------------------------------------------
# A coded byte b is a symbol only for b <= 26.  The contract for the rest: every frame decoder takes a received byte trit-wise as the
# reference's unpack3 does (b % 3, (b / 3) % 3, (b / 9) % 3), which is b mod 27; beacon-slot bytes are stepped over whatever they hold.
# "Lifting" a byte adds a multiple of 27 to it: the decode must not change.  CPU proof: test_noncanonical_semantics.py; GPU tests:
# test_gpu_noncanonical.py.
PINNED = (0, 1, 12, 13, 25)                        # dense: positions of block 0 of band 0 and of every band's last block that are always lifted
VALUES = 229                                       # 27 .. 255
# base stream (clean / sched / far<M> of Frame) and the pattern on top of it, per size; beacon framings add ("sched", "beacon")
LIFTS = {"full": (("sched", "dense"), ("sched", "sparse"), ("clean", "values"), ("far2", "dense"), ("far1000", "dense")),
         "padded": (("sched", "dense"), ("sched", "sparse"), ("clean", "values"), ("far2", "dense")),
         "small": (("sched", "dense"), ("sched", "sparse"), ("clean", "values"), ("far2", "dense"))}


def lift_rng(seed, name):
    import zlib
    return np.random.default_rng([int(seed), zlib.crc32(name.encode())])


def max_mult(b):
    """The largest j with b + 27 j <= 255"""
    return (255 - np.asarray(b, np.int64)) // 27


def block_index(L, cfg):
    """(blocks of all bands, 26): flat stream index of every coded symbol, band after band, block after block."""
    bi = body_index(L, cfg)
    assert len(bi) == 26 * sum(int(L.band_blocks[b]) for b in range(9))
    assert all(int(L.band_body_off[b]) == 26 * sum(int(L.band_blocks[q]) for q in range(b)) for b in range(9))
    return bi.reshape(-1, 26)


def band_first_block(L):
    return [int(L.band_body_off[b]) // 26 for b in range(9)]


def beacon_index(L, cfg):
    """Flat stream index of every beacon slot of the framed body (empty without a beacon)."""
    if not L.beacon_on:
        return np.zeros(0, np.int64)
    slot, period = int(cfg.beacon_band_slot), int(cfg.beacon_words_period)
    pos = np.arange(int(L.body_syms_framed), dtype=np.int64)
    return int(L.header_syms) + np.flatnonzero((pos >= slot) & ((pos - slot) % (9 * period) == 0))


def _dense(flat, at, rng, pinned=None):
    b = flat[at].astype(np.int64)
    j = rng.integers(0, max_mult(b) + 1)
    if pinned is not None:
        j = np.where(pinned, rng.integers(1, max_mult(b) + 1), j)
    flat[at] = b + 27 * j


def lift_bytes(flat, at, seed, name):
    """dense on arbitrary stream positions (a header, a whole COMPAT stream): b -> b + 27 j, j uniform in 0 .. max_mult(b)"""
    out = np.ascontiguousarray(flat, np.uint8).reshape(-1).copy()
    _dense(out, np.asarray(at, np.int64), lift_rng(seed, name))
    return out.reshape(np.shape(flat))


def lift(stream, L, cfg, pattern, seed, name, every=64, first=17):
    """stream (n, 9) -> the stream with bytes above 26, deterministic from (seed, name).
      dense   every body byte b -> b + 27 j, j uniform over 0 .. max_mult(b); at the PINNED positions of block 0 of band 0 and of every
              band's last block j >= 1, so that the places the tests assert are lifted whatever the seed.  Congruent mod 27.
      sparse  within each band only the blocks m with m % every == first carry one lifted byte, at position (m // every) % 26, by + 27
              and by the largest multiple that fits in turn.  Congruent mod 27.
      values  block i (counted over all bands): the byte at position i % 26 is overwritten with 27 + (i // 26) % 229, whatever was there:
              at most one symbol error per block.  For the clean stream.
      beacon  dense, and every beacon-slot byte a seeded random 0 .. 255."""
    flat = np.ascontiguousarray(stream, np.uint8).reshape(-1).copy()
    B = block_index(L, cfg); f0 = band_first_block(L); nb = [int(L.band_blocks[b]) for b in range(9)]
    rng = lift_rng(seed, name + "/" + pattern)
    if pattern in ("dense", "beacon"):
        pin = np.zeros(B.shape, bool)
        for r in [0] + [f0[b] + nb[b] - 1 for b in range(9) if nb[b]]:
            pin[r, list(PINNED)] = True
        _dense(flat, B.reshape(-1), rng, pin.reshape(-1))
        if pattern == "beacon":
            at = beacon_index(L, cfg)
            assert len(at), "no beacon slot in this framing"
            flat[at] = rng.integers(0, 256, len(at))
    elif pattern == "sparse":
        for b in range(9):
            m = np.arange(first, nb[b], every)
            at = B[f0[b] + m, (m // every) % 26]
            v = flat[at].astype(np.int64)
            flat[at] = v + 27 * np.where((m // every) % 2 == 1, max_mult(v), 1)
    elif pattern == "values":
        i = np.arange(len(B))
        flat[B[i, i % 26]] = 27 + (i // 26) % VALUES
    else:
        raise ValueError(pattern)
    return flat.reshape(-1, 9)


def lift_names(fr, what):
    """[(base, pattern)] of a frame at a size"""
    return LIFTS[what] + ((("sched", "beacon"),) if fr.L.beacon_on else ())


def lifted(fr, base, pattern):
    """-> (lifted stream, the stream under it, M = far rows in it, where they are)"""
    under, M, where = (fr.clean, 0, []) if base == "clean" else fr.stream(base)
    return lift(under, fr.L, fr.ocfg, pattern, fr.seed, "%s/%s" % (fr.name, base)), under, M, where


def values_pairs(n_blocks):
    """The (position, value) pairs `values` writes into a frame of n_blocks blocks."""
    i = np.arange(n_blocks)
    return set(zip((i % 26).tolist(), (27 + (i // 26) % VALUES).tolist()))
