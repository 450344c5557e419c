"""CPU tests of what FIXED (v6c) RS decoding means: a bounded-distance decoder.  ok <=> a codeword lies within t symbols of the block,
and then that codeword is the result.  Yardsticks: the original codeword below t; beyond t the codeword criterion of rs_patterns.py
(syndromes from table arithmetic, an exhaustive table of the syndromes of <= t errors for k = 24 and 22, the sphere-packing density
for k = 20 and 18) -- never a second decoder.  B1: the oracle's block decoder.  B2: the product's host block decoder.  B4: every
expectation of tests/test_gpu_fixed_errors.py, proven here with the oracle's frame decoder on the very streams the GPU test builds."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as ol
import rs_patterns as rp

KS = (24, 22, 20, 18)


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    return ge.load_package()


def random_codewords(orc, k, n, seed):
    rng = np.random.default_rng([seed, k])
    return orc.rs_encode_blocks(k, rng.integers(0, 27, size=(n, k), dtype=np.uint8), mode=1)


def test_helper_arithmetic_agrees_with_the_oracle(orc):
    """The helper's own tables: codewords of the oracle's FIXED encoder have zero syndromes, re-encoding detects exactly the rows whose
    syndromes are not zero, add / sub are inverse, the Vandermonde rows have the syndromes they were solved for."""
    F = rp.field(orc); rng = np.random.default_rng(3)
    a = np.arange(27)
    assert (F.sub[F.add[a[:, None], a[None, :]], a[None, :]] == a[:, None]).all()
    for k in KS:
        cw = random_codewords(orc, k, 3000, 1)
        assert rp.is_codeword(orc, k, cw).all()
        rows = cw.copy()
        hit = rng.random(len(rows)) < 0.5
        col = rng.integers(0, 26, len(rows))
        rows[hit, col[hit]] = F.add[rows[hit, col[hit]], rng.integers(1, 27, int(hit.sum()))]
        again = (orc.rs_encode_blocks(k, rows[:, :k], mode=1) == rows).all(axis=1)
        assert np.array_equal(rp.is_codeword(orc, k, rows), again) and np.array_equal(again, ~hit)
        assert len(rp.s0_rows(orc, k)) >= 50
        # syndromes are linear: S(c + e) = S(e)
        e = rp.canonical(k, 5)[0][:3000]
        assert np.array_equal(F.syndromes(F.add[cw[: len(e)], e], 26 - k), F.syndromes(e, 26 - k))


def test_schedule_contents():
    """What the schedule promises: every single error, every position pair, every value pair at (0, 25), >= 2000 sets per higher weight
    with the constructed placements, only blocks of >= 2 errors behind the weight-1 part, and full coverage once a band is long enough."""
    for k in KS:
        t = rp.tparam(k)
        rows, wt = rp.canonical(k, 11)
        assert wt.max() == t and rows.max() <= 26
        one = rows[wt == 1]
        assert len({(int(np.flatnonzero(r)[0]), int(r.max())) for r in one}) == 676
        if t >= 2:
            two = rows[wt == 2]
            assert len({tuple(np.flatnonzero(r)) for r in two}) == 325
            assert len({(int(r[0]), int(r[25])) for r in two if r[0] and r[25]}) == 676
            assert (wt[676 + rp.ZEROS:] >= 2).all()
        for w in range(3, t + 1):
            sets = {tuple(np.flatnonzero(r)) for r in rows[wt == w]}
            assert (wt == w).sum() >= 2000
            assert any(max(s) < k for s in sets) and any(min(s) >= k for s in sets)
            assert tuple(range(w)) in sets and tuple(range(26 - w, 26)) in sets
            assert any(k - 1 in s and k in s and max(s) - min(s) == w - 1 for s in sets)
        e, rec = rp.schedule(k, len(rows) + 2, 11)
        assert rec == rp.schedule_totals(k)
        rp.assert_coverage(k, rec)
        assert ((e != 0).sum(axis=1) <= t).all()
        assert (e[0] != 0).sum() == t and (e[0, :2] != 0).sum() == min(t, 2) and (e[-1] != 0).sum() == t and e[-1, k - 1] != 0
        short, rec = rp.schedule(k, 300, 11)
        with pytest.raises(AssertionError):
            rp.assert_coverage(k, rec)


def check_bounded_distance(orc, k, rows, decode):
    """decode(rows) -> (corrected rows, data, ok).  Every accepted row is a codeword within t symbols of its input and data = its first k."""
    cw, dk, ok = decode(rows)
    acc = ok == 1
    assert rp.is_codeword(orc, k, cw[acc]).all(), "accepted rows that are not codewords: %d of %d" % (int((~rp.is_codeword(orc, k, cw[acc])).sum()), int(acc.sum()))
    assert ((cw[acc] != rows[acc]).sum(axis=1) <= rp.tparam(k)).all()
    assert np.array_equal(dk[acc], cw[acc][:, :k])
    return acc


@pytest.mark.parametrize("k", KS)
def test_oracle_fixed_block_decoder_is_bounded_distance(orc, k):
    """B1.  Weight <= t: every schedule row on random codewords comes back as the original.  Weight t+1, t+2 and uniformly random words
    (200,000 each): every accepted row is a codeword within t of its input; k = 24, 22: accepted <=> the exhaustive syndrome table says a
    codeword is that near, row by row; k = 20, 18: the accepted share of random words is the sphere-packing density within 5 standard
    deviations (p = sum_{i<=t} C(26,i) 26^i / 27^R = 0.11853 and 0.024352).  Rows with syndromes (s, 0, .., 0) are rejected."""
    F = rp.field(orc); t = rp.tparam(k)
    dec = lambda rows: orc.rs_decode_blocks(k, rows, mode=1)
    for seed in (0, 1):
        e = np.concatenate([rp.canonical(k, seed)[0], [rp.forced_first(k, seed), rp.forced_last(k, seed)]])
        cw0 = random_codewords(orc, k, len(e), 20 + seed)
        cw, dk, ok = dec(F.add[cw0, e])
        assert ok.all() and np.array_equal(cw, cw0) and np.array_equal(dk, cw0[:, :k])
    b = rp.beyond_t(k)
    n = rp.POOL_N
    assert len(b["rows"]) == 2 * n >= 400_000
    assert ((b["rows"][:n] != 0).sum(axis=1) == t + 1).all() and ((b["rows"][n:] != 0).sum(axis=1) == t + 2).all()
    base = random_codewords(orc, k, 2 * n, 30)
    rng = np.random.default_rng([k, 31])
    pools = {"t+1 / t+2 on codewords": F.add[base, b["rows"]], "random words": rng.integers(0, 27, size=(n, 26), dtype=np.uint8)}
    for what, rows in pools.items():
        acc = check_bounded_distance(orc, k, rows, dec)
        if what != "random words":
            assert np.array_equal(acc, b["near"]), what              # the split the GPU tests use holds on other codewords than the zero word
        if t <= 2:
            assert np.array_equal(acc, rp.near_by_table(orc, k, rows)), what
        elif what == "random words":
            p = rp.sphere_density(k)
            assert abs(p - {20: 0.11853, 18: 0.024352}[k]) < 1e-5
            print("k=%d: %d of %d random words accepted, expected %.1f +- %.1f" % (k, acc.sum(), n, n * p, np.sqrt(n * p * (1 - p))))
            assert abs(int(acc.sum()) - n * p) <= 5 * np.sqrt(n * p * (1 - p)), (k, int(acc.sum()), n * p)
    s0 = F.add[base[: len(b["s0"])], b["s0"]]
    assert not dec(s0)[2].any() and not dec(b["s0"])[2].any()
    assert b["near"].sum() >= 200 and (~b["near"]).sum() >= 1000


@pytest.mark.parametrize("k", KS)
def test_host_block_decoder_is_bounded_distance(built, orc, k):
    """B2.  t3hip_rs_decode_block_host (mode 1; rs_correct of t3_rs_core.h, the block decoder the generic device path runs too), one block
    per call on a 20,000-row subsample of every pool of B1 plus all (s, 0, .., 0) rows: the verdict is the codeword criterion, accepted rows
    are codewords within t and carry the oracle's bytes."""
    F = rp.field(orc); lib = built.lib(); t = rp.tparam(k)
    fn = lib.t3hip_rs_decode_block_host
    fn.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p]

    def host(rows):
        cw = np.ascontiguousarray(rows, np.uint8).copy(); dk = np.zeros((len(cw), k), np.uint8); ok = np.zeros(len(cw), np.uint8)
        pc, pd = cw.ctypes.data, dk.ctypes.data
        for i in range(len(cw)):
            ok[i] = fn(k, 1, pc + 26 * i, pd + k * i)
        return cw, dk, ok
    b = rp.beyond_t(k); n = rp.POOL_N
    rng = np.random.default_rng([k, 41])
    e = np.concatenate([rp.canonical(k, 0)[0], [rp.forced_first(k, 0), rp.forced_last(k, 0)]])
    cw0 = random_codewords(orc, k, len(e), 42)
    cw, dk, ok = host(F.add[cw0, e])
    assert ok.all() and np.array_equal(cw, cw0) and np.array_equal(dk, cw0[:, :k])
    sub = np.sort(rng.choice(2 * n, 20_000, replace=False))
    base = random_codewords(orc, k, 20_000, 43)
    pools = {"t+1 / t+2": (F.add[base, b["rows"][sub]], b["near"][sub]),
             "random words": (rng.integers(0, 27, size=(20_000, 26), dtype=np.uint8), None),
             "(s, 0, .., 0)": (F.add[base[: len(b["s0"])], b["s0"]], np.zeros(len(b["s0"]), bool))}
    for what, (rows, near) in pools.items():
        acc = check_bounded_distance(orc, k, rows, host)
        ocw, odk, ook = orc.rs_decode_blocks(k, rows, mode=1)
        if near is None:
            near = rp.near_by_table(orc, k, rows) if t <= 2 else ook == 1       # (k = 20, 18: the oracle's verdict, proven in B1)
        assert np.array_equal(acc, near), what
        cw, dk, _ = host(rows)
        assert np.array_equal(cw[acc], ocw[acc]) and np.array_equal(dk[acc], odk[acc]), what


def plan_of(built, name):
    cfg = built.make_cfg(mode=1, **rp.CONFIGS[name])
    return lambda n_raw: built.plan(n_raw, cfg)


@pytest.mark.parametrize("name", sorted(rp.CONFIGS))
def test_gpu_expectations_hold_on_the_oracle(built, orc, name):
    """B4.  Every frame tests/test_gpu_fixed_errors.py decodes, built by the same functions, through the oracle's frame decoder: the <= t
    schedules (every band at its own t, coverage asserted) come back as the original pixels; near-only frames are accepted and differ from
    the original; frames with far blocks are refused.  A GPU run can then fail only because of a kernel."""
    plan = plan_of(built, name)
    for what in rp.CASES:
        fr = rp.make_frame(orc, plan, name, what)
        n_px = fr.n_px
        if what == "padded":
            assert n_px % 2 == 1 and all(fr.last_block_padded(b) for b in range(9))
        if what == "small":
            assert max(fr.blocks) < 52
        stream, rec = fr.sched()
        if what != "small":
            for b in range(9):
                rp.assert_coverage(fr.ks[b], rec[b])
        rc, px = orc.decode_frame(stream, ol.make_cfg(mode=1))
        assert rc == 0 and np.array_equal(px, fr.padded), (name, what)
        if what == "full":
            stream, placed = fr.near()
            assert all(v >= 200 for v in placed.values())
            rc, px = orc.decode_frame(stream, ol.make_cfg(mode=1))
            assert rc == 0 and len(px) == len(fr.padded) and not np.array_equal(px, fr.padded), (name, "near")
        assert ("near" in rp.CASES[what]) == (what == "full")
        for M in [int(c[3:]) for c in rp.CASES[what] if c.startswith("far")]:
            stream, M_, where = fr.stream("far%d" % M)
            assert len(where) == M and (0, 0) in where and (M == 1 or (8, fr.blocks[8] - 1) in where)
            if M > 2:
                assert all(v >= 50 for v in fr.s0_placed.values()) and set(fr.s0_placed) == set(fr.ks)
            rc, _ = orc.decode_frame(stream, ol.make_cfg(mode=1))
            assert rc != 0, (name, what, M)
            if name in rp.ONE_K and what != "small":      # the share of pixels in tiles that hold a far block, from the plan alone
                k = fr.ks[0]
                tiles = rp.far_tiles_one_k(k, where)
                p = built.window_plan(fr.n_raw, built.make_cfg(mode=1, **rp.CONFIGS[name]), len(fr.padded), 1, 0, 0, len(fr.padded), 1)
                assert p.tile_range == 1 and p.n_tiles == -(-max(fr.blocks) // 52)
                for tl in tiles[:3]:
                    x0 = tl * 108 * k; w = min(108 * k, len(fr.padded) - x0)
                    q = built.window_plan(fr.n_raw, built.make_cfg(mode=1, **rp.CONFIGS[name]), len(fr.padded), 1, x0, 0, w, 1)
                    assert (q.tile_lo, q.tile_hi) == (tl, tl + 1), (tl, q.tile_lo, q.tile_hi)
                outside = rp.pixels_outside_tiles(len(fr.padded), k, tiles).mean()
                assert 1.0 - outside <= 0.10 if M <= 2 else outside >= 0.40       # (the large frame: every other tile holds no far row)
