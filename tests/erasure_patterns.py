"""The yardstick of the erasure repair (include/t3hip.h, "repair with erasures"), and the damage plans its tests share (helper module,
no tests).

The rule: a received block y (26 bytes) with E = the positions whose byte is above 26, s = |E|, is ACCEPTED iff a codeword c of
RS(26, k) exists with 2 e + s <= r, e = the positions outside E where c differs from y; then the block becomes c.

The yardstick decides that without a locator found by Berlekamp-Massey, without a Chien search and without Forney -- on
rs_patterns.Field (table arithmetic, the syndromes, Gaussian elimination) only.  For every subset T of the positions outside E with
|T| <= (r - s) / 2, U = E + T, u = |U|:
  a codeword agrees with y outside U  <=>  the syndromes of y (any value standing in E) satisfy the recurrence of
  Lambda_U(x) = prod_{l in U} (1 - alpha^l x):  sum_{i = 0..u} lambda_i S_{j-i} = 0 for j = u .. r-1
  (=>: S_j = sum_{l in U} v_l X_l^{j+1}, and every X_l^-1 is a root of Lambda_U.  <=: u <= r, so the u x u Vandermonde system
  S_j = sum_l v_l X_l^{j+1}, j < u, has a solution v; the sequence it generates obeys the same recurrence of order u and agrees with
  S in its first u terms, hence in all r: y - v has zero syndromes.)
  The values at U come from Field.solve on that Vandermonde system.
Accepted iff some T passes (the codeword is unique: see the rule); s > r is a refusal.  All T of one size are tested at once with the
field tables: at most 2 626 subsets for r = 8 and s >= 1, 17 902 for s = 0.

The acceptance depends only on the additive error row and the mask (the scrambler subtracts a state from every trit, and the code is
linear), which gives expected_erasures(orc, fr, received) in the shape of test_repair_semantics.expected: blocks without a byte above 26
go through the oracle exactly as there, the others through the yardstick."""
import itertools

import numpy as np

import rs_patterns as rp


# ---- the yardstick --------------------------------------------------------------------------------------------------------------------
class Yardstick:
    def __init__(self, F):
        self.F = F
        self._lam = {}

    def _level(self, mask_bits, E, free, t):
        """(T (n, t), Lambda_U (n, s + t + 1)) for every t-subset T of `free`"""
        key = (mask_bits, t)
        hit = self._lam.get(key)
        if hit is not None:
            return hit
        F = self.F
        combos = list(itertools.combinations(free.tolist(), t))
        T = np.array(combos, np.int64).reshape(len(combos), t)
        U = np.concatenate([np.broadcast_to(E, (len(T), len(E))), T], axis=1)
        u = U.shape[1]
        lam = np.zeros((len(T), u + 1), np.uint8); lam[:, 0] = 1
        for q in range(u):                                                 # times (1 - alpha^l x)
            a = F.exp[U[:, q]].astype(np.uint8)
            lam[:, 1: q + 2] = F.sub[lam[:, 1: q + 2], F.mul[lam[:, 0: q + 1], a[:, None]]]
        if len(self._lam) > 256:
            self._lam = {k: v for k, v in self._lam.items() if k[0] == 0}   # keep the s = 0 tables (the large ones)
        self._lam[key] = (U, lam)
        return U, lam

    def decide(self, k, y, mask):
        """y (26,) symbols 0..26 (any value in the masked places), mask (26,) bool -> (accepted, the codeword or None)"""
        F = self.F; R = 26 - k
        y = np.asarray(y, np.uint8).reshape(26); mask = np.asarray(mask, bool).reshape(26)
        E = np.flatnonzero(mask); s = len(E)
        if s > R:
            return False, None
        S = F.syndromes(y[None, :], R)[0]
        free = np.flatnonzero(~mask)
        bits = int((mask.astype(np.int64) << np.arange(26)).sum())
        for t in range((R - s) // 2 + 1):
            U, lam = self._level(bits, E, free, t)
            u = s + t
            good = np.ones(len(U), bool)
            for j in range(u, R):
                acc = np.zeros(len(U), np.uint8)
                for i in range(u + 1):
                    acc = F.add[acc, F.mul[lam[:, i], S[j - i]]]
                good &= acc == 0
            hit = np.flatnonzero(good)
            if not len(hit):
                continue
            pos = U[hit[0]]
            c = y.copy()
            if u:
                V = np.array([[F.exp[((j + 1) * int(p)) % 26] for p in pos] for j in range(u)], np.uint8)
                c[pos] = F.sub[y[pos], F.solve(V, S[:u])]
            return True, c
        return False, None

    def decide_rows(self, k, Y, M):
        Y = np.asarray(Y, np.uint8).reshape(-1, 26); M = np.asarray(M, bool).reshape(-1, 26)
        ok = np.zeros(len(Y), bool); cw = Y.copy()
        for i in range(len(Y)):
            ok[i], c = self.decide(k, Y[i], M[i])
            if ok[i]:
                cw[i] = c
        return ok, cw


_yard = None


def yardstick(orc):
    global _yard
    if _yard is None:
        _yard = Yardstick(rp.field(orc))
    return _yard


def expected_erasures(orc, fr, received):
    """-> (R' flat, six words [0, uncorrectable blocks, blocks changed, bytes changed, flagged blocks, flagged blocks accepted], sorted
    [(band, block)] of the uncorrectable blocks).  Word 0: the header is not looked at here (the tests of the device entry leave it clean)."""
    F = rp.field(orc); L = fr.L; Y = yardstick(orc)
    rec = np.ascontiguousarray(received, np.uint8).reshape(-1)
    clean = fr.clean.reshape(-1)
    assert len(rec) == len(clean) == 9 * int(L.out_words)
    hs = int(L.header_syms)
    out = clean.copy()                                                    # beacon slots, tail: the encoder's bytes
    out[:hs] = rec[:hs]                                                   # the device entry never touches the header
    B = rp.block_index(L, fr.ocfg); f0 = rp.band_first_block(L)
    far = []; flagged = accepted = 0
    for b in range(9):
        k, nb = fr.ks[b], fr.blocks[b]
        idx = B[f0[b]: f0[b] + nb]
        hi = rec[idx] > 26
        e = F.sub[rec[idx] % 27, clean[idx]]
        tagged = hi.any(axis=1)
        rows = np.flatnonzero(e.any(axis=1) & ~tagged)                    # no byte above 26: the oracle, as test_repair_semantics.expected
        if len(rows):
            cw, _, ok = orc.rs_decode_blocks(k, e[rows], mode=1)
            good = ok == 1
            assert rp.is_codeword(orc, k, cw[good]).all() and ((cw[good] != e[rows[good]]).sum(axis=1) <= rp.tparam(k)).all()
            out[idx[rows[good]]] = F.add[clean[idx[rows[good]]], cw[good]]
            out[idx[rows[~good]]] = rec[idx[rows[~good]]]
            far += [(b, int(m)) for m in rows[~good]]
        for m in np.flatnonzero(tagged):                                  # the yardstick on (error row, mask)
            ok, cw = Y.decide(k, e[m], hi[m])
            flagged += 1
            if ok:
                accepted += 1
                out[idx[m]] = F.add[clean[idx[m]], cw]
            else:
                out[idx[m]] = rec[idx[m]]                                  # byte for byte as received, bytes above 26 included
                far.append((b, int(m)))
    diff = out != rec
    words = [0, len(far), int(diff[B].any(axis=1).sum()), int(diff[hs:].sum()), flagged, accepted]
    return out, words, sorted(far)


# ---- damage plans ---------------------------------------------------------------------------------------------------------------------
def admissible(k):
    """every (s, e) with 2 e + s <= r, s = 0 .. r"""
    r = 26 - k
    return [(s, e) for s in range(r + 1) for e in range((r - s) // 2 + 1)]


def beyond(k):
    """(s, e) with 2 e + s in {r + 1, r + 2}, and s in {r + 1, 26} without a further error"""
    r = 26 - k
    out = [(s, e) for s in range(r + 3) for e in range(r + 2) if 2 * e + s in (r + 1, r + 2) and s + e <= 26]
    return sorted(set(out + [(r + 1, 0), (26, 0)]))


def damage_rows(pairs, seed):
    """One row per (s, e) of `pairs`: (additive error values (n, 26) -- e of them nonzero, outside the mask --, mask (n, 26) with s set)"""
    rng = np.random.default_rng(seed)
    n = len(pairs)
    err = np.zeros((n, 26), np.uint8); mask = np.zeros((n, 26), bool)
    for i, (s, e) in enumerate(pairs):
        p = rng.permutation(26)
        mask[i, p[:s]] = True
        err[i, p[s: s + e]] = rng.integers(1, 27, e)
    return err, mask


class ByteSource:
    """Bytes above 26 for erased positions: every value 27..255 in turn; every fourth erased position instead a byte whose residue
    mod 27 is the clean symbol (right by chance on a real channel, here on purpose)."""

    def __init__(self, right=True):
        self.n = 0; self.seen = set(); self.right = self.wrong = 0; self.with_right = right

    def fill(self, clean_syms, mask):
        """clean_syms, mask (.., 26) -> bytes for the masked places (array of the mask's shape, 0 elsewhere)"""
        c = np.asarray(clean_syms, np.int64); out = np.zeros(c.shape, np.uint8)
        for at in zip(*np.nonzero(mask)):
            self.n += 1
            if self.with_right and self.n % 4 == 0:
                j = 1 + (self.n // 4) % int(rp.max_mult(c[at]))
                v = int(c[at]) + 27 * j
            else:
                v = 27 + (self.n * 5) % 229                                # 5 and 229 coprime: every value in turn
                while not self.with_right and v % 27 == c[at]:             # right=False: never right by chance either
                    self.n += 1
                    v = 27 + (self.n * 5) % 229
            out[at] = v; self.seen.add(v)
            if v % 27 == c[at]: self.right += 1
            else: self.wrong += 1
        return out


def block_pool(orc, k, pairs, seed, src=None):
    """Block-level cases without a scrambler: -> (clean codewords (n, 26), received bytes (n, 26), mask, additive error rows)"""
    F = rp.field(orc); rng = np.random.default_rng([seed, k])
    data = rng.integers(0, 27, (len(pairs), k)).astype(np.uint8)
    clean = orc.rs_encode_blocks(k, data, mode=1)
    assert rp.is_codeword(orc, k, clean).all()
    err, mask = damage_rows(pairs, [seed, k, 1])
    rec = F.add[clean, err]
    by = (src or ByteSource()).fill(clean, mask)
    rec = np.where(mask, by, rec).astype(np.uint8)
    return clean, rec, mask, err


def frame_kinds(k):
    """What the blocks of a band carry in turn: every admissible (s, e) (twice: positions differ), the beyond-capacity pairs, 'sched'
    rows of rs_patterns (s = 0, <= t errors) and clean blocks"""
    return admissible(k) * 2 + beyond(k) + ["sched"] * 6 + ["clean"] * 3


def damage_frame(orc, fr, seed, every=97, only=None, right=True, fill=True):
    """fr: rs_patterns.Frame -> (the received stream, flat; bool per block, band after band: the block carries a kind).  Per band the
    kinds of frame_kinds(k_b) (`only`: that list instead) sit in turn on its first and its last len(kinds) blocks and on every
    `every`-th block between; of the other blocks every fourth carries a <= t row of rs_patterns' schedule (no byte above 26), the rest
    are clean (fill=False: all of them clean).  Every beacon slot and every tail byte holds a byte above 26.  right=False: no erased byte
    with the right residue."""
    L = fr.L
    B = rp.block_index(L, fr.ocfg)
    clean = fr.clean.reshape(-1)
    errs = []; masks = []; planned = []
    for b in range(9):
        k, nb = fr.ks[b], fr.blocks[b]
        kinds = only if only is not None else frame_kinds(k)
        nk = len(kinds); m = np.arange(nb)
        idx = np.full(nb, -1, np.int64)
        mid = m % every == 0
        idx[mid] = (m[mid] // every + b) % nk
        idx[max(nb - nk, 0):] = (nb - 1 - m[max(nb - nk, 0):] + 3 * b) % nk
        idx[:nk] = (m[:nk] + 5 * b) % nk
        err = np.zeros((nb, 26), np.uint8); mask = np.zeros((nb, 26), bool)
        sched = rp.canonical(k, seed % 7)[0]
        rows = np.flatnonzero((idx < 0) & (m % 4 == 1) & fill)
        err[rows] = sched[(7 * rows + b) % len(sched)]
        at = np.flatnonzero(idx >= 0)
        mine = [kinds[i] for i in idx[at]]
        e2, m2 = damage_rows([x if isinstance(x, tuple) else (0, 0) for x in mine], [seed, b, nb])
        err[at] = e2; mask[at] = m2
        for j, x in zip(at, mine):
            if x == "sched":
                err[j] = sched[(7 * j + b) % len(sched)]
        errs.append(err); masks.append(mask); planned.append(idx >= 0)
    flat = rp.apply(orc, fr.clean, L, fr.ocfg, errs).reshape(-1).copy()
    mask = np.concatenate(masks)
    src = ByteSource(right)
    by = src.fill(clean[B], mask)
    flat[B[mask]] = by[mask]
    rng = np.random.default_rng([seed, 99])
    at = rp.beacon_index(L, fr.ocfg)
    flat[at] = rng.integers(27, 256, len(at))
    body_end = int(B.max()) + 1 if len(B) else int(L.header_syms)
    tail = np.arange(body_end, len(flat))
    tail = tail[~np.isin(tail, at)]
    flat[tail] = rng.integers(27, 256, len(tail))
    return flat, np.concatenate(planned)
