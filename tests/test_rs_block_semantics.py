"""CPU proof of what the block-level RS(26, k) decoders do over the full error range, in both arithmetics, and
t3hip_rs_decode_block_host -- rs_correct of t3_rs_core.h, the code the block kernels and the stage kernel run -- held to it.

Rows (rs_patterns.block_rows): FIXED codewords cw of seeded data plus, in the field, the whole <= t schedule, 3000 near rows and 3000
far rows (the 52 (s, 0, .., 0) rows first).  Syndromes are linear, so what a decoder does depends on e alone.

  FIXED   schedule: the codeword and the data back.  near: accepted, a codeword within t of the received row that is not cw.
          far: refused, the row as it came.
  COMPAT  schedule: accepted, and exactly cw + 2e = rx + e (the Forney sign of SURVEY 0.3), data = its first k symbols.  This closed
          form needs no decoder: it is the independent yardstick of the COMPAT arithmetic.
          beyond t: four classes.  Counts on the near / far rows (printed by test_compat_beyond_t_classes):

             k   rows          accepted-unchanged  accepted-modified  refused-untouched  refused-modified
            24   near (3000)                    0               3000                  0                 0
            24   far  (3000)                 2279                  0                721                 0
            22   near (3000)                    0               3000                  0                 0
            22   far  (3000)                 2568                236                196                 0
            20   near (3000)                    0               3000                  0                 0
            20   far  (3000)                 1335               1573                 53                39
            18   near (3000)                    0               3000                  0                 0
            18   far  (3000)                 1387               1531                 55                27
          refused-modified is the header's "on a 0 the reference leaves inout_n partially modified" (include/t3hip.h): rare, and met
          here on purpose."""
import ctypes as C

import numpy as np
import pytest

import rs_patterns as rp

KS = (24, 22, 20, 18)
GUARD = 0xA5
CLASSES = ("accepted-unchanged", "accepted-modified", "refused-untouched", "refused-modified")
MIN_REFUSED_MODIFIED = {20: 20, 18: 20}               # far rows; measured 39 and 27
MIN_FAR_ACCEPTED = 500                                # far rows COMPAT accepts, every k


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    return ge.load_package()


def classify(rx, out, ok):
    """-> index into CLASSES per row"""
    return np.where(ok == 1, 0, 2) + (out != rx).any(axis=1)


def compat_classes(orc, k):
    """-> {"near" | "far": counts in CLASSES order} of the oracle's COMPAT decoder"""
    B = rp.block_rows(k)
    out, _, ok = orc.rs_decode_blocks(k, B["rx"], mode=0)
    cls = classify(B["rx"], out, ok)
    return {p: np.bincount(cls[B[p]], minlength=4) for p in ("near", "far")}


@pytest.mark.parametrize("k", KS)
def test_fixed_full_range(orc, k):
    B = rp.block_rows(k); t = rp.tparam(k); rx, cw = B["rx"], B["cw"]
    assert len(rx[B["far"]]) == rp.BLOCK_POOL and len(rx[B["near"]]) >= 200, k
    out, dk, ok = orc.rs_decode_blocks(k, rx, mode=1)
    s, n, f = B["sched"], B["near"], B["far"]
    assert ok[s].all() and np.array_equal(out[s], cw[s]) and np.array_equal(dk[s], cw[s, :k]), k
    assert ok[n].all() and rp.is_codeword(orc, k, out[n]).all(), k
    assert ((out[n] != rx[n]).sum(axis=1) <= t).all() and (out[n] != cw[n]).any(axis=1).all(), k
    assert np.array_equal(dk[n], out[n, :k]), k
    assert not ok[f].any() and np.array_equal(out[f], rx[f]), k


@pytest.mark.parametrize("k", KS)
def test_compat_schedule_closed_form(orc, k):
    B = rp.block_rows(k); F = rp.field(orc); s = B["sched"]
    want = F.add[B["rx"][s], B["e"][s]]                                   # cw + 2e
    assert np.array_equal(want, F.add[B["cw"][s], F.add[B["e"][s], B["e"][s]]])
    out, dk, ok = orc.rs_decode_blocks(k, B["rx"][s], mode=0)
    assert ok.all() and np.array_equal(out, want) and np.array_equal(dk, want[:, :k]), k


def test_compat_beyond_t_classes(orc):
    print("%3s  %-12s %s" % ("k", "rows", "  ".join(CLASSES)))
    for k in KS:
        got = compat_classes(orc, k)
        for p in ("near", "far"):
            print("%3d  %-4s (%4d)  %s" % (k, p, got[p].sum(), "  ".join("%*d" % (len(c), v) for c, v in zip(CLASSES, got[p]))))
        far = got["far"]
        assert far.sum() == rp.BLOCK_POOL
        assert far[0] + far[1] >= MIN_FAR_ACCEPTED, (k, far)
        assert far[3] >= MIN_REFUSED_MODIFIED.get(k, 0), (k, far)
        assert far[2] >= 1, (k, far)


@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("k", KS)
def test_host_block_decoder_is_the_oracle(built, orc, k, mode):
    """t3hip_rs_decode_block_host on every row: return value and the 26 bytes in/out are the oracle's; data_k is the first k symbols on
    a 1 and keeps its guard pattern on a 0.  On the schedule the expectation is the closed form of each arithmetic, not the oracle."""
    B = rp.block_rows(k); F = rp.field(orc); rx = B["rx"]
    fn = built.lib().t3hip_rs_decode_block_host
    fn.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    code = np.ascontiguousarray(rx).copy(); dk = np.full((len(rx), k + 2), GUARD, np.uint8); ok = np.zeros(len(rx), np.int64)
    pc, pd = code.ctypes.data, dk.ctypes.data
    for i in range(len(rx)):
        ok[i] = fn(k, mode, pc + 26 * i, pd + (k + 2) * i + 1)
    want, wdk, wok = orc.rs_decode_blocks(k, rx, mode=mode)
    s = B["sched"]
    closed = B["cw"][s] if mode == 1 else F.add[rx[s], B["e"][s]]
    assert (ok[s] == 1).all() and np.array_equal(code[s], closed) and np.array_equal(dk[s, 1: k + 1], closed[:, :k]), (k, mode)
    assert np.array_equal(ok, wok) and np.array_equal(code, want), (k, mode)
    acc = ok == 1
    assert np.array_equal(dk[acc, 1: k + 1], code[acc, :k]) and np.array_equal(dk[acc, 1: k + 1], wdk[acc]), (k, mode)
    assert (dk[~acc] == GUARD).all() and (dk[:, 0] == GUARD).all() and (dk[:, k + 1] == GUARD).all(), (k, mode)
    if mode == 0 and k in MIN_REFUSED_MODIFIED:                            # the partially modified rows went through it
        assert ((code != rx).any(axis=1) & ~acc).sum() >= MIN_REFUSED_MODIFIED[k]
