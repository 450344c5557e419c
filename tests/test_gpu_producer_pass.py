"""The syndrome stage of the fused FIXED decoders takes three K-steps: a lane's 13th symbol (block positions 12 and 25) rides in the spare
byte of step 0 (csrc/t3_decode_fx2.h, fx2_set; tests/test_synd_operand3.py is the host model of the operand), and the pixel kernels hold
two steps of the operand in registers.  Here: FIXED frames of two full decoder tiles plus a ragged third one (a tile is 8,640 pixels at 52
blocks per band; 2 x 8,640 + 1,235 pixels, an odd count) through decode_fixed_px_kernel (single-frame entry, pixels and RGB) and through
dec_frames_px (the batch entry, two frames in one launch: a workgroup's next tile may belong to the other frame), pixels and both verdict
words against the oracle's decoder on the same bytes.

  single     RS(26,20): every single error (position 0..25 x magnitude 1..26, parity positions included), one per block; the stream's
             first block clean
  first0 / first1 / first12 / first25
             the stream's first block (whose symbols 0 and 1 see the scrambler's pre-period states) with a single error at that position;
             every other block two or three errors, one of them at position 12 or 25 -- the symbol that moved; one block with four
             errors, which the verdict counts
  lifted     the frame `first12` with a byte above 26 at position 12 of every fourth block and at position 25 of every fourth block (the
             non-canonical unpack path meets the inserted bytes): congruent mod 27, so the same pixels and verdict
  k24 / k22 / k18
             one frame per other code, 0..t errors per block

The expectation is built as in tests/test_gpu_fx3.py: the oracle's block decoder on the error row alone tells whether a block is refused
(its data stay as received, verdict word 1 counts it) or moved by a codeword; the original stream plus those codewords is a clean stream
whose decode by the oracle's frame decoder is the expected output, and where nothing is refused the oracle's frame decoder is also run on
the corrupted bytes themselves."""
import functools

import numpy as np
import pytest

import oracle_lib as ol
import rs_patterns as rp
from test_gpu_frames import decode_batch, decode_loop, oracle_batch

pytestmark = pytest.mark.gpu
N_PX = 2 * 8640 + 1235
N_FRAMES = 2
PROFILE = {24: 0, 22: 1, 20: 2, 18: 3}
K20_CASES = ("single", "first0", "first1", "first12", "first25", "lifted")


def error_rows(orc, case, k, L, rng):
    """Per band an (band_blocks, 26) array of additive errors for the case."""
    t = (26 - k) // 2
    errs = [np.zeros((int(L.band_blocks[b]), 26), np.uint8) for b in range(9)]
    g = 0                                                                            # block number over all bands
    for b in range(9):
        for m in range(len(errs[b])):
            e = errs[b][m]
            if case == "single":
                if g >= 1:
                    i = (g - 1) % 676; e[i // 26] = i % 26 + 1
            elif case.startswith("first") or case == "lifted":
                p0 = 12 if case == "lifted" else int(case[5:])
                if g == 0:
                    e[p0] = int(rng.integers(1, 27))
                else:
                    c = 4 if g == 333 else 2 + g % 2
                    first = (12, 25)[(g // 2) % 2]
                    while True:
                        pos = [first] + [int(p) for p in rng.permutation(26) if p != first][: c - 1]
                        e[:] = 0; e[pos] = rng.integers(1, 27, c)
                        if c < 4 or orc.rs_decode_blocks(k, e[None], 1)[2][0] == 0:     # the four-error block: one that is refused, not miscorrected
                            break
            else:                                                                    # another code: 0..t errors per block, positions 12 / 25 favoured
                c = int(rng.integers(0, t + 1))
                first = (12, 25, int(rng.integers(0, 26)))[g % 3]
                pos = ([first] + [int(p) for p in rng.permutation(26) if p != first])[:c]
                e[pos] = rng.integers(1, 27, c)
            g += 1
    return errs


@functools.lru_cache(maxsize=None)
def frames(case, k):
    """-> (corrupted streams, expected pixel records, refused blocks) of N_FRAMES frames: computed once, shared, never written to."""
    import __graft_entry__ as ge
    t3 = ge.load_package()
    orc = ol.oracle()
    pr = PROFILE[k]
    cfg = t3.make_cfg(mode=1, profile=pr, uep=pr); ocfg = lambda: ol.make_cfg(mode=1, profile=pr, uep=pr)
    n_raw = (N_PX + 1) // 2; L = t3.plan(n_raw, cfg)
    n_blocks = sum(int(L.band_blocks[b]) for b in range(9))
    assert n_blocks >= 677 and min(int(L.band_blocks[b]) for b in range(9)) > 2 * 52, "every single-error pattern, and a third tile"
    px, coded = oracle_batch(N_FRAMES, N_PX, 1, pr)
    bad, want, refused = [], [], []
    for f in range(N_FRAMES):
        rng = np.random.default_rng([4100 + f, k, K20_CASES.index(case) if case in K20_CASES else 9])
        errs = error_rows(orc, case, k, L, rng)
        moved, M = [], 0
        for e in errs:
            _, dk, ok = orc.rs_decode_blocks(k, e, 1)
            data = np.where(ok[:, None] != 0, dk, e[:, :k])                           # refused: the data symbols stay as received
            moved.append(orc.rs_encode_blocks(k, data, 1)); M += int((ok == 0).sum())
        stream = rp.apply(orc, coded[f].reshape(-1, 9), L, cfg, errs).reshape(-1).copy()
        clean = rp.apply(orc, coded[f].reshape(-1, 9), L, cfg, moved)
        if case == "lifted":
            at = rp.block_index(L, cfg)
            for p, r in ((12, 0), (25, 2)):
                idx = at[r::4, p]
                stream[idx] = stream[idx] + 27 * (1 + (np.arange(len(idx)) % 8))      # b <= 26: at most 26 + 216
            assert (stream[at[0::4, 12]] > 26).all() and (stream[at[2::4, 25]] > 26).all()
        rc, opx = orc.decode_frame(clean, ocfg()); assert rc == 0 and len(opx) == 2 * n_raw
        if M == 0:
            rc, direct = orc.decode_frame(stream.reshape(-1, 9), ocfg()); assert rc == 0 and np.array_equal(direct, opx)
            assert np.array_equal(opx[:N_PX], px[f])
        else:
            assert orc.decode_frame(stream.reshape(-1, 9), ocfg())[0] == t3.E_RS
        stream.setflags(write=False); opx.setflags(write=False)
        bad.append(stream); want.append(opx); refused.append(M)
    four = case.startswith("first") or case == "lifted"
    assert all(M == (1 if four else 0) for M in refused), (case, refused)
    return bad, want, refused


def check(gpu, orc, case, k):
    bad, want, refused = frames(case, k)
    pr = PROFILE[k]
    cfg = gpu.make_cfg(mode=1, profile=pr, uep=pr); n_raw = (N_PX + 1) // 2
    ver_want = [v for M in refused for v in (0, M)]
    expect = {gpu.FRAMES_PIXELS: [w.view(np.uint8).reshape(-1) for w in want], gpu.FRAMES_RGB: [orc.quant_to_rgb(w) for w in want]}
    for fmt in (gpu.FRAMES_PIXELS, gpu.FRAMES_RGB):
        out, ver = decode_loop(gpu, bad, n_raw, fmt, cfg)                              # decode_fixed_px_kernel
        assert ver == ver_want, (case, fmt, "single", ver, ver_want)
        assert all(np.array_equal(a, b) for a, b in zip(out, expect[fmt])), (case, fmt, "single")
        p, seen, out, ver = decode_batch(gpu, bad, n_raw, fmt, cfg, 4096 + 16)         # dec_frames_px, one launch
        assert p.one_launch == 1 and ver == ver_want, (case, fmt, "batch", ver, ver_want)
        assert all(np.array_equal(a, b) for a, b in zip(out, expect[fmt])), (case, fmt, "batch")


@pytest.mark.parametrize("case", K20_CASES)
def test_rs26_20(gpu, orc, case):
    check(gpu, orc, case, 20)


@pytest.mark.parametrize("k", [24, 22, 18])
def test_other_codes(gpu, orc, k):
    check(gpu, orc, "upto_t", k)
