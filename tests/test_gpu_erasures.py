"""GPU tests of the repair with erasures (include/t3hip.h, "repair with erasures"): erasure_fixed_kernel<R> and erasure_generic_kernel
against expected_erasures of tests/erasure_patterns.py -- built on rs_patterns.Field and the oracle only, proven on the CPU in
tests/test_erasure_semantics.py --, the profile entries, and the block-level device entry against the host entry and the yardstick.
The buffer after a repair equals the expectation byte for byte, the six verdict words are the yardstick's, and the bytes in front of and
behind the frame's 9 * n_in bytes are untouched (tests/bounds.py).  Byte work: every comparison is exact."""
import functools

import numpy as np
import pytest

import bounds
import erasure_patterns as ep
import oracle_lib as ol
import rs_patterns as rp
from test_erasure_semantics import KS, beyond_pool, constructed_pool, host_decode
from test_repair_semantics import FUSED, GENERIC

pytestmark = pytest.mark.gpu
FILL = bounds.FILLS[0]
SWEEP = FUSED + GENERIC
SEED = {"small": 31, "padded": 32}


@functools.lru_cache(maxsize=4)
def _frame(name, what):
    import __graft_entry__ as ge
    t3 = ge.load_package()
    cfg = t3.make_cfg(mode=1, **rp.CONFIGS[name])
    return rp.make_frame(ol.oracle(), lambda n_raw: t3.plan(n_raw, cfg), name, what)


@functools.lru_cache(maxsize=4)
def _damaged(name, what):
    """(received, expected, six words, planned blocks) of a configuration at a size: computed once, shared, never written"""
    fr = _frame(name, what); orc = ol.oracle()
    s, planned = ep.damage_frame(orc, fr, SEED[what])
    exp, words, far = ep.expected_erasures(orc, fr, s)
    for a in (s, exp):
        a.setflags(write=False)
    return s, exp, words, planned


def run(gpu, fr, stream, flags, offset=0, fill=FILL, era=True):
    """One repair call on a guarded copy of `stream` -> (the frame's bytes afterwards, the verdict words: six with era, else the plain
    entry's four); the guards are checked, every byte of the frame may change."""
    import torch
    b = np.ascontiguousarray(stream, np.uint8).reshape(-1)
    buf = bounds.Buf(len(b), fill, offset, data=b, name="frame", may_change=((0, len(b)),))
    ver = torch.full((8,), 7, dtype=torch.int32, device="cuda")
    cfg = gpu.make_cfg(mode=1, **fr.kw)
    fn = gpu.repair_erasures_frame_async if era else gpu.repair_frame_async
    fn(buf.ptr, len(b) // 9, cfg, fr.n_raw, flags, ver.data_ptr(), torch.cuda.current_stream().cuda_stream)
    bounds.sync()
    v = ver.cpu().tolist()
    assert v[6 if era else 4:] == [7] * (2 if era else 4), "words behind the verdict were written"
    return buf.result(), v[: 6 if era else 4]


# ---- the main sweep ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ("small", "padded"))
@pytest.mark.parametrize("name", SWEEP)
def test_erasure_sweep(gpu, orc, name, what):
    """Every framing at two sizes, the damage plan of erasure_patterns.damage_frame: buffer = expected, words = the yardstick's, guards
    untouched, at base offsets 0 and 2 mod 16; a dry run gives the same words and stores nothing; a second run changes nothing."""
    fr = _frame(name, what)
    assert gpu.repair_plan(fr.n_raw, gpu.make_cfg(mode=1, **fr.kw)).path == (1 if name in FUSED else 0)
    s, exp, words, planned = _damaged(name, what)
    tag = (name, what)
    assert (s > 26).any() and words[4] > 0
    if what == "padded":                                                   # the plan's coverage
        B = rp.block_index(fr.L, fr.ocfg); f0 = rp.band_first_block(fr.L)
        e_res = rp.field(orc).sub[s[B] % 27, fr.clean.reshape(-1)[B]]
        for b in range(9):
            rows = slice(f0[b], f0[b] + fr.blocks[b])
            hi = (s[B[rows]] > 26).sum(axis=1); er = ((e_res[rows] != 0) & (s[B[rows]] <= 26)).sum(axis=1)
            have = set(zip(hi.tolist(), er.tolist()))
            assert have >= set(ep.admissible(fr.ks[b])) | set(ep.beyond(fr.ks[b])), (tag, b)
            assert ((hi == 0) & (er == 0)).any() and ((hi == 0) & (er > 1)).any(), (tag, b)
        assert 0 < words[5] < words[4] and words[1] >= words[4] - words[5], tag
        assert (s[rp.beacon_index(fr.L, fr.ocfg)] > 26).all()
    for offset in (0, 2):
        got, ver = run(gpu, fr, s, gpu.REPAIR_WRITE, offset)
        assert ver == words, (tag, offset, "words", ver, words)
        bounds.check_equal(got, exp, FILL, "repaired %s at %d" % (tag, offset))
    got, ver = run(gpu, fr, s, 0)                                           # the same words, no byte stored
    assert ver == words, (tag, "dry run", ver, words)
    assert np.array_equal(got, s), (tag, "dry run wrote")
    got, ver = run(gpu, fr, exp, gpu.REPAIR_WRITE)                          # the repaired frame: nothing left to change
    refused_flagged = words[4] - words[5]
    assert ver == [0, words[1], 0, 0, refused_flagged, 0], (tag, "second repair", ver)
    assert np.array_equal(got, exp), (tag, "second repair wrote")


def test_other_fill_and_offset(gpu, orc):
    """The second fill of tests/bounds.py: a byte the kernel never wrote, or a result that depends on a byte outside the frame, shows."""
    for name in ("k18", "four_codes"):
        fr = _frame(name, "small")
        s, exp, words, _ = _damaged(name, "small")
        got, ver = run(gpu, fr, s, gpu.REPAIR_WRITE, offset=2, fill=bounds.FILLS[1])
        assert ver == words, (name, ver, words)
        bounds.check_equal(got, exp, bounds.FILLS[1], "repaired %s" % name)


# ---- the tile loop ----------------------------------------------------------------------------------------------------------------------
def test_tile_loop(gpu, orc):
    """One k20 frame of 9 x CU count + 1 fused tiles, as test_gpu_repair.test_tile_loop builds it, so that every workgroup walks its
    loop more than twice; the damage plan thinned to every 701st block of a band (the yardstick runs on the CPU)."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    tiles = 9 * cus + 1
    n_px = tiles * 108 * 20 - 1001                                          # the last tile ragged, the count odd
    cfg = gpu.make_cfg(mode=1, **rp.CONFIGS["k20"])
    fr = rp.Frame(orc, lambda n_raw: gpu.plan(n_raw, cfg), "k20", n_px, 103)
    p = gpu.repair_plan(fr.n_raw, cfg)
    assert p.path == 1 and p.n_tiles >= 3 * 3 * cus and p.blocks_per_tile == 9 * 52
    s, planned = ep.damage_frame(orc, fr, 33, every=701)
    exp, words, far = ep.expected_erasures(orc, fr, s)
    f0 = rp.band_first_block(fr.L)
    at = np.concatenate([np.flatnonzero(planned[f0[b]: f0[b] + fr.blocks[b]]) // 52 for b in range(9)])     # the tiles that hold a planned block
    assert all(((at >= lo) & (at < lo + 3 * cus)).sum() > 100 for lo in (0, 3 * cus, 6 * cus)) and words[5] > 500   # in every pass of the loop
    got, ver = run(gpu, fr, s, gpu.REPAIR_WRITE)
    assert ver == words, (ver, words)
    bounds.check_equal(got, exp, FILL, "tile loop")


# ---- no byte above 26: the plain repair ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ("small", "padded"))
@pytest.mark.parametrize("name", SWEEP)
def test_without_flagged_bytes_is_the_plain_repair(gpu, orc, name, what):
    """On the streams of rs_patterns.CASES (no byte above 26) the buffer and words [0..3] are t3hip_repair_frame_async's, [4] = [5] = 0."""
    fr = _frame(name, what)
    for case in rp.CASES[what] + ("clean",):
        s = fr.clean if case == "clean" else fr.stream(case)[0]
        assert not (np.asarray(s) > 26).any()
        want, w4 = run(gpu, fr, s, gpu.REPAIR_WRITE, era=False)
        got, w6 = run(gpu, fr, s, gpu.REPAIR_WRITE)
        assert w6 == w4 + [0, 0], (name, what, case, w6, w4)
        assert np.array_equal(got, want), (name, what, case)
        if case == "clean":
            assert w6 == [0] * 6 and np.array_equal(got, np.asarray(s).reshape(-1))


# ---- the contrast: what the mod-27 rule throws away ---------------------------------------------------------------------------------------
def test_flagged_bytes_are_recoverable(gpu, orc):
    """A k20 frame whose damaged blocks each hold 4..6 flagged bytes and no other error.  (The flagged bytes' residues are wrong, and of
    the seeded candidates a block stays damaged only where the oracle's errors-only decoder refuses the residues: a pattern of 4..6
    symbol errors may lie within t = 3 of ANOTHER codeword.)  The plain repair reports every such block uncorrectable and the decoder
    reports failures; the new entry returns the clean frame, which decodes to the frame's pixels with verdict [0, 0]."""
    import torch
    fr = _frame("k20", "padded")
    cfg = gpu.make_cfg(mode=1, **fr.kw)
    F = rp.field(orc)
    s, planned = ep.damage_frame(orc, fr, 34, every=5, only=[(4, 0), (5, 0), (6, 0)], right=False, fill=False)
    clean = fr.clean.reshape(-1)
    B = rp.block_index(fr.L, fr.ocfg)
    s[int(B.max()) + 1:] = clean[int(B.max()) + 1:]                          # (no beacon; the tail stays clean here: the plain words below count blocks only)
    e = F.sub[s[B] % 27, clean[B]]
    rows = np.flatnonzero((s[B] > 26).any(axis=1))
    _, _, ok = orc.rs_decode_blocks(20, e[rows], mode=1)
    back = rows[ok == 1]
    s[B[back]] = clean[B[back]]                                             # the errors-only rule accepts these residues: not part of the contrast
    rows = rows[ok != 1]
    hi = (s[B[rows]] > 26).sum(axis=1)
    assert len(rows) > 1000 and set(hi.tolist()) == {4, 5, 6} and not (s[B[rows]] % 27 == clean[B[rows]])[s[B[rows]] > 26].any()
    assert np.array_equal(np.flatnonzero((s != clean).reshape(-1)), np.sort(B[rows][s[B[rows]] > 26]))   # flagged bytes and nothing else
    n = len(fr.padded); st = torch.cuda.current_stream().cuda_stream

    def decode(stream):
        d = torch.from_numpy(np.ascontiguousarray(stream).reshape(-1).copy()).cuda()
        ver = torch.full((2,), 7, dtype=torch.int32, device="cuda")
        out = torch.full((6 * n + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        got = gpu.decode_frame_async(d.data_ptr(), d.numel() // 9, cfg, fr.n_raw, out.data_ptr(), n, ver.data_ptr(), True, st)
        bounds.sync()
        return got, ver.cpu().tolist(), out[: 6 * n].cpu().numpy().view(ol.PIXEL_DT)

    got, w4 = run(gpu, fr, s, gpu.REPAIR_WRITE, era=False)
    assert w4 == [0, len(rows), 0, 0] and np.array_equal(got, s), w4         # every damaged block uncorrectable, nothing repaired
    cnt, ver, _ = decode(s)
    assert cnt == n and ver[0] == 0 and ver[1] > 0, ver                      # the decoder reports failures
    got, w6 = run(gpu, fr, s, gpu.REPAIR_WRITE)
    assert w6 == [0, 0, len(rows), int(hi.sum()), len(rows), len(rows)], w6
    bounds.check_equal(got, clean, FILL, "flagged bytes recovered")
    cnt, ver, px = decode(got)
    assert cnt == n and ver == [0, 0] and np.array_equal(px, fr.padded)


# ---- the synchronous entries ------------------------------------------------------------------------------------------------------------
def _damage_header(stream, n):
    """n symbol errors in the header's first RS(26,18) block (t = 4)"""
    s = np.ascontiguousarray(stream, np.uint8).copy().reshape(-1)
    at = np.arange(n) * 2 + 1
    s[at] = (s[at] + 1 + np.arange(n) % 25) % 27
    return s


@pytest.mark.parametrize("name", ("k20", "k20_beacon83"))
def test_profile_entries(gpu, orc, name):
    """A damaged but decodable header is rewritten; counts and return codes follow the plain entries' test."""
    import torch
    fr = _frame(name, "small")
    cfg = gpu.make_cfg(mode=1, **fr.kw)
    hdr = gpu.header_encode(cfg, fr.n_raw)
    assert np.array_equal(fr.clean.reshape(-1)[: len(hdr)], hdr)
    n_in = len(fr.clean)
    within, _ = ep.damage_frame(orc, fr, 35, only=ep.admissible(fr.ks[0]))
    mixed = _damaged(name, "small")[0]
    cases = (("header+2", _damage_header(within, 2), gpu.OK, True), ("header+9", _damage_header(within, 9), gpu.E_HEADER, False),
             ("mixed", np.array(mixed), gpu.E_RS, False), ("mixed, header+2", _damage_header(mixed, 2), gpu.E_RS, True))
    for label, s, want_rc, hdr_fixed in cases:
        exp, words, _ = ep.expected_erasures(orc, fr, s)
        assert want_rc == gpu.E_HEADER or (words[1] > 0) == (want_rc == gpu.E_RS), (label, words)   # (the plan of `mixed` holds refused blocks)
        if hdr_fixed:
            exp = exp.copy(); exp[: len(hdr)] = hdr                          # ... and the header comes back as t3hip_header_encode's bytes
        if want_rc == gpu.E_HEADER:
            exp, words = s, [0] * 6                                          # nothing written
        for flags in (gpu.REPAIR_WRITE, 0):
            tag = (name, label, flags)
            buf = bounds.Buf(len(s), FILL, 0, data=s, name="frame", may_change=((0, len(s)),))
            rc, counts = gpu.repair_erasures_profile_dev(buf.ptr, n_in, gpu.DecoderContext(mode=1).cfg_last_seen, flags, torch.cuda.current_stream().cuda_stream)
            bounds.sync()
            assert rc == want_rc and counts == [1 if hdr_fixed else 0] + words[1:], (tag, rc, counts, words)
            bounds.check_equal(buf.result(), exp if flags else s, FILL, "profile_dev %s" % (tag,))
            w = s.copy().reshape(-1, 9)
            rc, counts = gpu.repair_erasures_profile(w, gpu.DecoderContext(mode=1), flags)
            assert rc == want_rc and counts == [1 if hdr_fixed else 0] + words[1:], (tag, "host", rc, counts)
            assert np.array_equal(w.reshape(-1), exp if flags else s), (tag, "host")
    with pytest.raises(gpu.T3Error) as e:                                     # seen->mode must be FIXED on entry
        gpu.repair_erasures_profile(np.array(mixed).reshape(-1, 9), gpu.DecoderContext(mode=0))
    assert e.value.code == gpu.E_ARG


# ---- block level --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
def test_block_entries(gpu, orc, k):
    """t3hip_rs_decode_blocks_erasures_dev and its host-buffer form on the pools of the CPU test: the host entry's verdicts and blocks,
    which that test holds to the yardstick; a refused block and its data row untouched."""
    import torch
    rec = np.concatenate([constructed_pool(k)[1], beyond_pool(k)[1]])
    n = len(rec)
    ok, out, data = host_decode(gpu, k, rec)
    yok, ycw = ep.yardstick(orc).decide_rows(k, rec % 27, rec > 26)
    assert np.array_equal(ok, yok) and np.array_equal(out[ok], ycw[ok]) and ok[: len(constructed_pool(k)[1])].all() and not ok.all()
    code = bounds.Buf(26 * n, FILL, 0, data=rec, name="code", may_change=((0, 26 * n),))
    d_data = bounds.Buf(k * n, FILL, 0, name="data"); d_ok = bounds.Buf(n, FILL, 0, name="ok")
    gpu.rs_decode_blocks_erasures_dev(k, code.ptr, n, d_data.ptr, d_ok.ptr, torch.cuda.current_stream().cuda_stream)
    bounds.sync()
    got_ok = d_ok.result()
    assert np.array_equal(got_ok, ok.astype(np.uint8)), k
    bounds.check_equal(code.result(), out, FILL, "blocks in place")
    got_data = d_data.result().reshape(n, k)
    assert np.array_equal(got_data[ok], out[ok, :k]) and (got_data[~ok] == FILL).all(), k
    c2, d2, ok2 = gpu.rs_decode_blocks_erasures(k, rec, np.full((n, k), 0x5A, np.uint8))
    assert np.array_equal(ok2, ok.astype(np.uint8)) and np.array_equal(c2, out), k
    assert np.array_equal(d2[ok], out[ok, :k]) and (d2[~ok] == 0x5A).all(), k
