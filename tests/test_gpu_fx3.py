"""The RS(26,20) pixel kernels correct their queued blocks in closed form (csrc/t3_decode_fx3.h: two or three errors from determinants,
Berlekamp-Massey behind a wave-uniform branch for everything else; tests/test_fx3_closed_form.py is the proof on the CPU).  Here: FIXED
frames of three decoder tiles plus a ragged end -- 3 x 2,160 + 7 pixels, and one more for the odd-pixel pad -- whose blocks ALL carry a
given error load, through the single-frame entry and the batch entry with two frames, pixels and RGB out:

  two      every block exactly 2 errors          three    every block exactly 3
  upto3    0..3 per block                        upto5    0..5 per block: refused and miscorrected blocks among them

A third of the blocks is hit at position 0, a third at position 25, a third at a parity position (then wherever the seed says).  The
yardstick is the oracle's decoder.  An additive error on the wire is the same error on the descrambled block (tests/rs_patterns.py,
apply), and the code is linear, so the oracle's block decoder run on the error row alone tells what a decoder makes of the block: refused
(counted in verdict word 1; the data symbols stay as received), or moved by a codeword (zero unless miscorrected).  Adding that codeword's
re-encoding to the original stream gives a clean stream whose decode by the oracle's frame decoder is the expected output, pixel for pixel;
where no block is refused the oracle's frame decoder is also run on the corrupted stream itself.  The same frames go through RS(26,22)
(R = 4, loads of its own t) and through the raw-word kernel, which keep Berlekamp-Massey alone."""
import functools

import numpy as np
import pytest

import oracle_lib as ol
import rs_patterns as rp
from test_gpu_frames import decode_batch, decode_loop, oracle_batch

pytestmark = pytest.mark.gpu
SIZES = [3 * 2160 + 7, 3 * 2160 + 8]
LOADS = {"two": (2, 2), "three": (3, 3), "upto3": (0, 3), "upto5": (0, 5)}
LOADS_K22 = {"two": (2, 2), "upto2": (0, 2), "upto4": (0, 4)}
N_FRAMES = 2


def error_rows(n_blocks, lo, hi, rng):
    """(n_blocks, 26) additive errors, lo..hi per block; block i's first error at position 0 / 25 / a parity position for i % 3 = 0 / 1 / 2."""
    e = np.zeros((n_blocks, 26), np.uint8)
    for i in range(n_blocks):
        c = int(rng.integers(lo, hi + 1))
        first = (0, 25, int(rng.integers(20, 25)))[i % 3]
        perm = [first] + [int(p) for p in rng.permutation(26) if p != first]
        e[i, perm[:c]] = rng.integers(1, 27, c)
    return e


@functools.lru_cache(maxsize=None)
def case(profile, n_px, load):
    """-> (corrupted streams, expected pixel records per frame, refused blocks per frame): computed once, shared, never written to."""
    import __graft_entry__ as ge
    t3 = ge.load_package()
    orc = ol.oracle(); F = rp.field(orc)
    k = {2: 20, 1: 22}[profile]
    lo, hi = (LOADS if k == 20 else LOADS_K22)[load]
    cfg = t3.make_cfg(mode=1, profile=profile, uep=profile); ocfg = lambda: ol.make_cfg(mode=1, profile=profile, uep=profile)
    n_raw = (n_px + 1) // 2; L = t3.plan(n_raw, cfg)
    px, coded = oracle_batch(N_FRAMES, n_px, 1, profile)
    bad, want, refused = [], [], []
    for f in range(N_FRAMES):
        rng = np.random.default_rng(9000 + 100 * f + 10 * hi + lo)
        errs = [error_rows(int(L.band_blocks[b]), lo, hi, rng) for b in range(9)]
        moved, M = [], 0
        for e in errs:
            _, dk, ok = orc.rs_decode_blocks(k, e, 1)
            data = np.where(ok[:, None] != 0, dk, e[:, :k])                       # refused: the data symbols stay as received
            moved.append(orc.rs_encode_blocks(k, data, 1)); M += int((ok == 0).sum())
        stream = rp.apply(orc, coded[f].reshape(-1, 9), L, cfg, errs)
        clean = rp.apply(orc, coded[f].reshape(-1, 9), L, cfg, moved)
        rc, opx = orc.decode_frame(clean, ocfg()); assert rc == 0 and len(opx) == 2 * n_raw
        if M == 0:
            rc, direct = orc.decode_frame(stream, ocfg()); assert rc == 0 and np.array_equal(direct, opx)
        else:
            assert orc.decode_frame(stream, ocfg())[0] == t3.E_RS
        if hi <= (26 - k) // 2:
            assert M == 0 and np.array_equal(opx[:n_px], px[f])
        stream = stream.reshape(-1).copy(); stream.setflags(write=False); opx.setflags(write=False)
        bad.append(stream); want.append(opx); refused.append(M)
    if hi > (26 - k) // 2:
        assert min(refused) > 0 and any(not np.array_equal(w[:n_px], p) for w, p in zip(want, px)), "no refused / miscorrected block in the load"
    return bad, want, refused


def check(gpu, orc, profile, n_px, load, fmts):
    bad, want, refused = case(profile, n_px, load)
    cfg = gpu.make_cfg(mode=1, profile=profile, uep=profile); n_raw = (n_px + 1) // 2
    ver_want = [v for M in refused for v in (0, M)]
    expect = {gpu.FRAMES_PIXELS: [w.view(np.uint8).reshape(-1) for w in want], gpu.FRAMES_RGB: [orc.quant_to_rgb(w) for w in want],
              gpu.FRAMES_WORDS: [np.asarray(orc.pack_pixels(w)).reshape(-1) for w in want]}
    for fmt in fmts:
        out, ver = decode_loop(gpu, bad, n_raw, fmt, cfg)                          # the single-frame entry
        assert ver == ver_want, (load, fmt, "single", ver, ver_want)
        assert all(np.array_equal(a, b) for a, b in zip(out, expect[fmt])), (load, fmt, "single")
        if fmt != gpu.FRAMES_WORDS:                                                # the batch entry, one launch
            p, seen, out, ver = decode_batch(gpu, bad, n_raw, fmt, cfg, 4096 + 16)
            assert p.one_launch == 1 and ver == ver_want, (load, fmt, "batch", ver, ver_want)
            assert all(np.array_equal(a, b) for a, b in zip(out, expect[fmt])), (load, fmt, "batch")


@pytest.mark.parametrize("load", sorted(LOADS))
@pytest.mark.parametrize("n_px", SIZES)
def test_closed_form_pixel_kernels(gpu, orc, n_px, load):
    """RS(26,20): decode_fixed_px_kernel<6, *, false> and dec_frames_px<6, *, false> -- pixels and both verdict words against the oracle."""
    check(gpu, orc, 2, n_px, load, (gpu.FRAMES_PIXELS, gpu.FRAMES_RGB))


@pytest.mark.parametrize("load", sorted(LOADS))
def test_raw_word_kernel_unchanged(gpu, orc, load):
    """The same frames as raw words: decode_fixed_kernel keeps fx2_correct."""
    check(gpu, orc, 2, SIZES[0], load, (gpu.FRAMES_WORDS,))


@pytest.mark.parametrize("load", sorted(LOADS_K22))
@pytest.mark.parametrize("n_px", SIZES)
def test_r4_pixel_kernels_unchanged(gpu, orc, n_px, load):
    """The same pixels coded with RS(26,22): the R = 4 pixel kernels keep fx2_correct."""
    check(gpu, orc, 1, n_px, load, (gpu.FRAMES_PIXELS, gpu.FRAMES_RGB))
