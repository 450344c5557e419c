"""CPU proof of what the frame decoders owe a received byte above 26, and of every expectation of tests/test_gpu_noncanonical.py.

The contract: a coded byte b is taken trit-wise, as the reference's unpack3 does (b % 3, (b / 3) % 3, (b / 9) % 3) -- that is b mod 27 --
in the header and in the body, FIXED and COMPAT; beacon-slot bytes are stepped over whatever they hold.  The reference itself indexes
past its tables with such a byte, so the yardstick is the oracle (oracle/t3_oracle.c) and never the reference.

Proven here, on the very streams the GPU tests build (rs_patterns.lift): the oracle's answer to a lifted stream is its answer to
lifted % 27 -- code, pixels or words, the configuration it saw, the word count -- and is the original frame where the stream under the
lifting decodes, T3_E_RS where it holds far rows; the streams reach the places where a kernel's reduction can go wrong; and two wrong
reductions, applied to the same streams, are refused or give other pixels, so the streams tell mod 27 from them."""
import zlib

import numpy as np
import pytest

import oracle_lib as ol
import rs_patterns as rp

E_RS = -6                                          # include/t3hip.h; the oracle answers with the same codes
SIZES = ("full", "padded", "small")
COMPAT_NAMES = ["p3_uniform20", "p2_luma", "p5_tile64_luma", "p2_beacon83", "p1_beacon3_slot8", "p5_tile7x5_mixed4"]


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    return ge.load_package()


def oracle_frame(orc, stream):
    seen = ol.make_cfg(mode=1)
    rc, px = orc.decode_frame(stream, seen)
    return rc, px, seen.as_dict()


def same_answer(a, b):
    return a[0] == b[0] and a[2] == b[2] and ((a[1] is None and b[1] is None) or np.array_equal(a[1], b[1]))


def clamp26(s):
    """A wrong reduction: saturate"""
    return np.minimum(s, 26)


def sub27_once(s):
    """A wrong reduction: subtract 27 once.  What it leaves is no symbol wherever the byte was >= 54"""
    return np.where(s >= 27, s - 27, s).astype(np.uint8)


def test_patterns_are_what_they_say():
    """max_mult is the largest multiple that fits a byte; `values` covers all 26 x 229 (position, value) pairs once a frame holds 5954
    blocks and not one block earlier; what the two wrong reductions of the controls do to a byte."""
    b = np.arange(27)
    assert (b + 27 * rp.max_mult(b) <= 255).all() and (b + 27 * (rp.max_mult(b) + 1) > 255).all()
    assert len(rp.values_pairs(26 * rp.VALUES)) == 26 * rp.VALUES == 5954
    assert len(rp.values_pairs(26 * rp.VALUES - 1)) == 5953
    v = np.array(sorted(rp.values_pairs(5954)))
    assert set(v[:, 0]) == set(range(26)) and set(v[:, 1]) == set(range(27, 256))
    s = np.arange(256, dtype=np.uint8)
    assert (sub27_once(s) % 27 == s % 27).all() and (sub27_once(s)[54:] > 26).all() and (clamp26(s)[27:] == 26).all()


@pytest.mark.parametrize("what", SIZES)
@pytest.mark.parametrize("name", sorted(rp.CONFIGS))
def test_lifted_frames_on_the_oracle(built, orc, name, what):
    """Every framing at its three sizes, every stream of rp.lift_names: where the streams are lifted (asserted, not assumed), what the
    oracle makes of them, and the two controls on every dense stream.  Saturating at 26 goes to the oracle as it is.  Subtracting 27
    once leaves a byte congruent mod 27, which the oracle -- reducing mod 27 itself -- would decode like the original: what makes it wrong
    is that it leaves non-symbols, so that is asserted (more than t of them in some block of every band), and the oracle gets them
    saturated, as a table lookup clamped to its last entry would see them."""
    cfg = built.make_cfg(mode=1, **rp.CONFIGS[name])
    fr = rp.make_frame(orc, lambda n_raw: built.plan(n_raw, cfg), name, what)
    L = fr.L
    B = rp.block_index(L, fr.ocfg); f0 = rp.band_first_block(L); nb = fr.blocks
    last = [f0[b] + nb[b] - 1 for b in range(9) if nb[b]]
    slots = rp.beacon_index(L, fr.ocfg)
    names = rp.lift_names(fr, what)
    assert (name in ("k22_beacon2_slot8", "k20_beacon83")) == (("sched", "beacon") in names) == bool(len(slots))
    if what == "padded":
        assert all(fr.last_block_padded(b) for b in range(9))
    for base, pattern in names:
        s, under, M, where = rp.lifted(fr, base, pattern)
        again, _, _, _ = rp.lifted(fr, base, pattern)
        assert np.array_equal(s, again), "not deterministic"
        sf, uf = s.reshape(-1), np.ascontiguousarray(under).reshape(-1)
        hi = sf > 26
        body = np.zeros(len(sf), bool); body[B.reshape(-1)] = True
        other = ~body; other[slots] = False
        assert uf.max() <= 26 and np.array_equal(sf[other], uf[other])             # header, padding: as they were
        label = (name, what, base, pattern)
        if pattern in ("dense", "beacon"):
            assert np.array_equal(sf[body] % 27, uf[body]), label
            assert hi[B[0, :2]].all(), label                                       # the pre-period scrambler states
            assert hi[B[0, list(rp.PINNED)]].all() and hi[B[last][:, list(rp.PINNED)]].all(), label     # 12 | 13, 25; every band's last block
            assert 0.8 < hi[body].mean() < 0.95, label                              # j = 0 is one of 9 or 10 values
            if what != "small":                                                    # the seam between the two lanes of a block, either side alone
                assert (~hi[B[:, 12]] & hi[B[:, 13]]).any() and (hi[B[:, 12]] & ~hi[B[:, 13]]).any(), label
            if base == "sched":
                assert (hi & (uf != fr.clean.reshape(-1))).any(), label             # an error position that is lifted too
            if pattern == "beacon":
                assert (sf[slots] != uf[slots]).mean() > 0.9, label
                assert hi[slots].mean() > 0.8 and len(np.unique(sf[slots])) > min(len(slots), 256) // 2, label
        elif pattern == "sparse":
            assert np.array_equal(sf % 27, uf), label
            per_block = hi[B].sum(axis=1)
            want = np.zeros(len(B), np.int64)
            for b in range(9):
                want[f0[b] + np.arange(17, nb[b], 64)] = 1
            assert np.array_equal(per_block, want), label
            if what != "small":
                assert want.sum() >= 9 and (hi & (uf != fr.clean.reshape(-1))).any(), label
                lifted_by = (sf[hi].astype(int) - uf[hi]) // 27
                assert (lifted_by == 1).any() and (sf[hi] > 228).any(), label       # + 27, and the largest multiple that fits
            if name in rp.ONE_K and what != "small":
                assert all(hi[B[:, p]].any() for p in range(26)), label             # 66 * 52 blocks per band: every position
        else:
            assert base == "clean" and np.array_equal(sf[~hi], uf[~hi]) and (hi[B].sum(axis=1) == 1).all(), label
            got = {(int(np.flatnonzero(hi[B[i]])[0]), int(sf[B[i]][hi[B[i]]][0])) for i in range(len(B))}
            assert got == rp.values_pairs(len(B)), label
            if what != "small":
                if name in rp.ONE_K:
                    assert min(nb) >= rp.MIN_BLOCKS_ONE_K and len(got) == 26 * rp.VALUES, label
                assert {p for p, _ in got} == set(range(26)) and {v for _, v in got} == set(range(27, 256)), label
                print("%s %s: %d of 5954 (position, value) pairs" % (name, what, len(got)))
            assert hi[B[0, 0]] and hi[B[last][:, :]].any(axis=1).all(), label
        # the oracle: lifted == lifted % 27, and what the stream under it must decode to
        a = oracle_frame(orc, s)
        b = oracle_frame(orc, (s % 27).astype(np.uint8))
        assert same_answer(a, b), label
        if M == 0:
            assert a[0] == 0 and np.array_equal(a[1], fr.padded) and len(a[1]) == 2 * fr.n_raw, label
            assert a[2] == oracle_frame(orc, fr.clean)[2], label
        else:
            assert a[0] == E_RS and len(where) == M, label
        if pattern in ("dense", "beacon"):
            for wrong in (clamp26, sub27_once):
                w = wrong(s)
                if wrong is sub27_once:                                             # congruent, but not symbols: what a table sees is not 0 .. 26
                    assert all((w.reshape(-1)[B[f0[b]: f0[b] + nb[b]]] > 26).sum(axis=1).max() > rp.tparam(fr.ks[b]) for b in range(9) if nb[b]), label
                    w = clamp26(w)
                rc, px, _ = oracle_frame(orc, w)
                assert rc != 0 or not np.array_equal(px, fr.padded), (label, wrong.__name__)


@pytest.mark.parametrize("name", sorted(rp.CONFIGS))
def test_lifted_headers_on_the_oracle(built, orc, name):
    """One header byte lifted, and all of them: the same configuration, word count and pixels as the clean stream."""
    cfg = built.make_cfg(mode=1, **rp.CONFIGS[name])
    fr = rp.make_frame(orc, lambda n_raw: built.plan(n_raw, cfg), name, "small")
    want = oracle_frame(orc, fr.clean)
    assert want[0] == 0 and np.array_equal(want[1], fr.padded)
    for hdr in header_lifts(fr):
        assert not np.array_equal(hdr, fr.clean) and np.array_equal(hdr % 27, fr.clean)
        assert same_answer(oracle_frame(orc, hdr), want), name


def header_lifts(fr):
    """[one header byte lifted by the largest multiple that fits, all header bytes lifted by 27 j, j >= 1] (shared with the GPU tests)"""
    hs = int(fr.L.header_syms)
    one = fr.clean.copy().reshape(-1); one[5] += 27 * int(rp.max_mult(one[5]))
    every = fr.clean.copy().reshape(-1)
    rng = rp.lift_rng(fr.seed, fr.name + "/header")
    every[:hs] = every[:hs] + 27 * rng.integers(1, rp.max_mult(every[:hs]) + 1)
    return [one.reshape(-1, 9), every.reshape(-1, 9)]


def compat_streams(orc, name, nbws=(26, 600, 5000)):
    """The COMPAT streams the GPU test decodes: (nbw, corrupt, stream, the stream lifted `dense`, header included)"""
    from test_gpu_parity import CFGS
    from test_oracle_vs_ref import decoder_consistent_stream
    rng = np.random.default_rng(zlib.crc32(name.encode()) + 27)
    kw = dict(CFGS[name])
    if isinstance(kw.get("uep"), list):
        kw["uep"] = [x % 3 for x in kw["uep"]]
    ocfg = ol.make_cfg(**kw)
    for nbw in nbws:
        for corrupt in (0, 1, 5):
            s = decoder_consistent_stream(orc, rng, ocfg, nbw, corrupt)
            yield nbw, corrupt, s, rp.lift_bytes(s, np.arange(s.size), 7, "%s/%d/%d" % (name, nbw, corrupt))


@pytest.mark.parametrize("name", COMPAT_NAMES)
def test_lifted_compat_streams_on_the_oracle(orc, name):
    """COMPAT: streams its decoder accepts, 0 / 1 / 5 corruptions, every byte (header included) lifted: the same code, words and
    configuration as unlifted."""
    for nbw, corrupt, s, up in compat_streams(orc, name):
        assert np.array_equal(up % 27, s) and (up > 26).mean() > 0.8
        sa, sb = ol.make_cfg(), ol.make_cfg()
        ra, a = orc.decode_profile(up, sa)
        rb, b = orc.decode_profile(s, sb)
        assert ra == rb and np.array_equal(a, b) and sa.as_dict() == sb.as_dict(), (name, nbw, corrupt)
        if corrupt == 0:
            assert ra == 0 and len(a) > 0
