"""Bodies for the stage-3 entry (t3hip_demap_rsdecode_bands[_dev], stage_decode_kernel) across its workgroup steps (helper module, no
tests): the numpy restatement of OLD:948-993 the stage tests share, the lattice of body sizes x beacons x codes x byte offsets, the
planted-failure sets and the schedule body.  tests/test_stage_shapes_lattice.py asserts that the lattice reaches every edge the kernel
has; tests/test_gpu_stage_steps.py runs it.

The kernel works in runs of STEP = 64 blocks per band: workgroup g = nine waves, wave b = blocks [64 g, 64 g + 64) of band b.  Every
band but the beacon band has nb = n_words // 26 blocks; the beacon band has fewer, so its wave leaves the last workgroups early.  The
run is staged at the 16-byte phase of the body, each wave's output at the 16-byte phase of its destination."""
import numpy as np

import rs_patterns as rp

KS = [24, 22, 20, 18]
STEP = 64                                          # kStageBlocks

CODESETS = [  # (code_k, code_mode): every code, mixed k, COMPAT, FIXED, mixed modes
    (KS, (0, 0, 0, 0)), (KS, (1, 1, 1, 1)), (KS, (0, 1, 0, 1)), ([20, 20, 20, 20], (1, 0, 0, 1)), ([18, 24, 22, 20], (1, 1, 0, 0)),
]
UEPS = [[0, 1, 2, 3, 0, 1, 2, 3, 1], [2] * 9, [3, 3, 0, 0, 1, 1, 2, 2, 3]]


# ---- the restatement -------------------------------------------------------------------------------------------------
def band_columns(body, hdr):
    """OLD:950-961: band b = slot b of every word, minus the words wi % period == 0 of the beacon slot."""
    body = np.asarray(body, np.uint8).reshape(-1, 9)
    skip = bool(hdr.beacon_enabled) and hdr.beacon_words_period > 0
    cols = []
    for b in range(9):
        col = body[:, b]
        if skip and hdr.beacon_band_slot == b:
            col = col[np.arange(len(body)) % hdr.beacon_words_period != 0]
        cols.append(col)
    return cols


def restate_stage3(orc, body, hdr, code_k=KS, code_mode=(0, 0, 0, 0)):
    """OLD:948-993 -> (ok, out_syms): per band (code band_profile[b] % 4) whole blocks decoded in order; at the first block that does
    not decode, False with the symbols of the blocks before it."""
    out = []
    for b, col in enumerate(band_columns(body, hdr)):
        q = hdr.band_profile[b] % 4
        k, nblk = code_k[q], len(col) // 26
        if not nblk:
            continue
        _, dk, okv = orc.rs_decode_blocks(k, col[: 26 * nblk], mode=code_mode[q])
        bad = np.flatnonzero(okv == 0)
        if len(bad):
            out.append(dk[: bad[0]].reshape(-1))
            return False, np.concatenate(out)
        out.append(dk.reshape(-1))
    return True, (np.concatenate(out) if out else np.zeros(0, np.uint8))


def band_offsets(n_words, hdr, code_k):
    """Output offset of each band's first block, and the total."""
    off, o = [], 0
    for b, col in enumerate(band_columns(np.zeros((n_words, 9), np.uint8), hdr)):
        off.append(o)
        o += (len(col) // 26) * code_k[hdr.band_profile[b] % 4]
    return off, o


def band_words(n_words, hdr, b):
    """The words whose slot b holds band b's symbols, in order."""
    w = np.arange(n_words)
    skip = bool(hdr.beacon_enabled) and hdr.beacon_words_period > 0
    return w[w % hdr.beacon_words_period != 0] if skip and hdr.beacon_band_slot == b else w


def stage_body(orc, rng, hdr, code_k, code_mode, n_words, corrupt=0):
    """A descrambled body whose band columns are codewords of the band's code (FIXED parity, which the COMPAT decoder also passes
    when clean), tails random, corrupt: up to that many symbol errors in ~30 % of the blocks."""
    body = rng.integers(0, 27, size=(n_words, 9), dtype=np.uint8)
    for b in range(9):
        rows = band_words(n_words, hdr, b)
        k = code_k[hdr.band_profile[b] % 4]
        nblk = len(rows) // 26
        if not nblk:
            continue
        data = rng.integers(0, 27, size=(nblk, k), dtype=np.uint8)
        cw = orc.rs_encode_blocks(k, data, mode=1)
        if corrupt:
            hit = np.flatnonzero(rng.random(nblk) < 0.3)
            for e in range(corrupt):
                sel = hit[rng.random(len(hit)) < (1.0 if e == 0 else 0.5)]
                pos = rng.integers(0, 26, len(sel))
                cw[sel, pos] = (cw[sel, pos] + rng.integers(1, 27, len(sel))) % 27
        body[rows[: 26 * nblk], b] = cw.reshape(-1)
    return body


# ---- the geometry of plan_stages (t3_api_stages.cpp), restated ---------------------------------------------------------------
def geometry(n_words, uep, beacon, code_k):
    """-> dict: k[9], blocks[9], off[9], total, bcn_band (9: none) -- arithmetic on the counts, no columns built."""
    period, slot, enabled = beacon
    skip = bool(enabled) and period > 0
    bcn = slot if skip and slot < 9 else 9
    k, blocks, off, total = [], [], [], 0
    for b in range(9):
        kb = code_k[uep[b] % 4]
        syms = n_words - (n_words + period - 1) // period if b == bcn else n_words
        k.append(kb); blocks.append(syms // 26); off.append(total); total += blocks[-1] * kb
    return dict(k=k, blocks=blocks, off=off, total=total, bcn_band=bcn)


# ---- the lattice ---------------------------------------------------------------------------------------------------------
NBS = (63, 64, 65, 127, 128, 129, 193)              # blocks of a non-beacon band: both sides of one, two and three workgroup steps
TAILS = (0, 11, 25)                                 # words behind the last whole block
BEACONS = ((0, 0, 0), (1, 4, 1), (2, 0, 1), (2, 8, 1), (3, 4, 1), (83, 0, 1), (83, 8, 1))
CORRUPT = (0, 1, 3, 5)


def lattice():
    """147 cases: every (nb, tail, beacon); code set, band codes, corruption level and the two byte offsets rotate over them, each with
    its own stride so that they vary independently of each other."""
    cases, i = [], 0
    for nb in NBS:
        for r in TAILS:
            for bcn in BEACONS:
                cases.append(dict(i=i, nb=nb, n_words=26 * nb + r, beacon=bcn, codeset=i % 5, uep=(i // 5) % 3, corrupt=CORRUPT[i % 4],
                                  in_off=i % 16 + 16 * (i % 3), out_off=(5 * i + i // 16) % 16 + 16 * (i % 2)))
                i += 1
    return cases


def case_geometry(c):
    return geometry(c["n_words"], UEPS[c["uep"]], c["beacon"], CODESETS[c["codeset"]][0])


def case_body(orc, make_cfg, c):
    """-> (hdr, code_k, code_mode, body): seeded by the case number"""
    code_k, code_mode = CODESETS[c["codeset"]]
    hdr = make_cfg(uep=UEPS[c["uep"]], beacon=c["beacon"])
    body = stage_body(orc, np.random.default_rng([20261021, c["i"]]), hdr, code_k, code_mode, c["n_words"], c["corrupt"])
    return hdr, code_k, code_mode, body


# ---- planted failures ------------------------------------------------------------------------------------------------------
PLANT_NB, PLANT_TAIL, PLANT_BEACON, PLANT_UEP = 129, 11, (3, 4, 1), UEPS[0]
PLANT_WORDS = 26 * PLANT_NB + PLANT_TAIL
PLANT_OFFS = (0, 7, 54)


def plant_sets(blocks):
    """name -> [(band, block)] for the per-band block counts of the planted body"""
    last = blocks[8] - 1
    return {
        "a_min_in_last_workgroup": [(0, 128), (8, 3)],
        "b_same_band_two_workgroups": [(2, 70), (2, 5)],
        "c_beacon_wave_twice_and_later_band": [(4, 66), (4, 70), (6, 10)],
        "d_first_block": [(0, 0)],
        "e_last_block_of_last_band": [(8, last)],
        "f_every_band": [(b, (37 * b + 11) % blocks[b]) for b in range(9)],
    }


def refused_row(orc, rng, k, mode):
    """A word the band's decoder does not take, found by search in the band's own arithmetic."""
    while True:
        junk = rng.integers(0, 27, 26, dtype=np.uint8)
        if not orc.rs_decode_blocks(k, junk, mode=mode)[2][0]:
            return junk


def plant(body, hdr, b, m, row):
    """Block m of band b := row, in place."""
    w = band_words(len(body), hdr, b)[26 * m: 26 * m + 26]
    assert len(w) == 26
    body[w, b] = row


# ---- the schedule body -------------------------------------------------------------------------------------------------------
SCHED_WORDS = 26 * (rp.schedule_len(18) + 2)
SCHED_UEP, SCHED_BEACON = UEPS[0], (83, 8, 1)


def schedule_body(orc, make_cfg):
    """Nine bands, each the whole rp.canonical schedule of its own k cycled to the band's block count, on FIXED codewords of seeded data.
    -> dict hdr, body, geo, data[9] (blocks, k), rx[9], e[9] (blocks, 26)"""
    F = rp.field(orc); rng = np.random.default_rng(20261022)
    hdr = make_cfg(uep=SCHED_UEP, beacon=SCHED_BEACON)
    geo = geometry(SCHED_WORDS, SCHED_UEP, SCHED_BEACON, KS)
    body = rng.integers(0, 27, size=(SCHED_WORDS, 9), dtype=np.uint8)
    data, rx, err = [], [], []
    for b in range(9):
        k, nblk = geo["k"][b], geo["blocks"][b]
        rows = rp.canonical(k, 0)[0]
        assert nblk >= len(rows)
        e = rows[np.arange(nblk) % len(rows)]
        d = rng.integers(0, 27, size=(nblk, k), dtype=np.uint8)
        r = F.add[orc.rs_encode_blocks(k, d, mode=1), e]
        body[band_words(SCHED_WORDS, hdr, b)[: 26 * nblk], b] = r.reshape(-1)
        data.append(d); rx.append(r); err.append(e)
    return dict(hdr=hdr, body=body, geo=geo, data=data, rx=rx, e=err)


def schedule_far_blocks(geo):
    """Two blocks per band for the far rows: one in the band's first half, one in its last workgroup."""
    return [(b, m) for b in range(9) for m in ((211 * (b + 1)) % (geo["blocks"][b] // 2), geo["blocks"][b] - 1 - b)]
