"""The block-level decoders t3hip_rs_decode_blocks[_dev] (rs_decode_blocks_kernel) over the full error range in both arithmetics, on the
rows of tests/test_rs_block_semantics.py: FIXED codewords plus the whole <= t schedule, 3000 near rows and 3000 far rows per code, in one
launch per (k, mode) -- some 10 000 blocks, dozens of 256-lane steps -- and in slices of 255, 256 and 257 blocks; code, data and ok
buffers at odd byte offsets between guard bytes.

Expected, per row (proven with the oracle, and the oracle pinned to the reference, on the CPU):
  FIXED   schedule: the original codeword (closed form).  near: the oracle's codeword.  far: refused, the row as it came.
  COMPAT  schedule: cw + 2e (closed form).  beyond t: the oracle's row, the partially modified rows of refused blocks included.
  both    data = the first k symbols of an accepted row; data_k of a refused block keeps its guard pattern."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle_lib as ol
import rs_patterns as rp

pytestmark = pytest.mark.gpu
KS = (24, 22, 20, 18)
G_CODE, G_DATA, G_OK = 0xC3, 0xA5, 0xEE
OFF_CODE, OFF_DATA, OFF_OK, PAD = 3, 1, 5, 32                              # odd byte offsets; PAD guard bytes behind


@functools.lru_cache(maxsize=None)
def expected(k, mode):
    """-> (rx, code afterwards, ok) for all rows of rp.block_rows(k)"""
    orc = ol.oracle(); F = rp.field(orc); B = rp.block_rows(k)
    rx, s, n, f = B["rx"], B["sched"], B["near"], B["far"]
    code, _, ok = orc.rs_decode_blocks(k, rx, mode=mode)
    code = code.copy(); ok = ok.copy()
    if mode == 1:
        code[s] = B["cw"][s]; ok[s] = 1
        assert ok[n].all() and rp.is_codeword(orc, k, code[n]).all()       # (tests/test_rs_block_semantics.py proves the rest)
        code[f] = rx[f]; ok[f] = 0
    else:
        code[s] = F.add[rx[s], B["e"][s]]; ok[s] = 1
    return rx, code, ok


def run_dev(t3, k, mode, rx):
    import torch
    n = len(rx)
    hc = np.full(OFF_CODE + 26 * n + PAD, G_CODE, np.uint8); hc[OFF_CODE: OFF_CODE + 26 * n] = rx.reshape(-1)
    d_code = torch.from_numpy(hc).cuda()
    d_data = torch.full((OFF_DATA + k * n + PAD,), G_DATA, dtype=torch.uint8, device="cuda")
    d_ok = torch.full((OFF_OK + n + PAD,), G_OK, dtype=torch.uint8, device="cuda")
    t3.rs_decode_blocks_dev(k, mode, d_code.data_ptr() + OFF_CODE, n, d_data.data_ptr() + OFF_DATA, d_ok.data_ptr() + OFF_OK,
                            torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    code, data, ok = d_code.cpu().numpy(), d_data.cpu().numpy(), d_ok.cpu().numpy()
    for a, off, ln, g in ((code, OFF_CODE, 26 * n, G_CODE), (data, OFF_DATA, k * n, G_DATA), (ok, OFF_OK, n, G_OK)):
        assert (a[:off] == g).all() and (a[off + ln:] == g).all()          # nothing written outside the three ranges
    return code[OFF_CODE: OFF_CODE + 26 * n].reshape(n, 26), data[OFF_DATA: OFF_DATA + k * n].reshape(n, k), ok[OFF_OK: OFF_OK + n]


def check(k, mode, rows, got, what):
    rx, want, wok = expected(k, mode)
    code, data, ok = got
    assert np.array_equal(ok, wok[rows]), (k, mode, what)
    assert np.array_equal(code, want[rows]), (k, mode, what)
    acc = ok == 1
    assert np.array_equal(data[acc], want[rows][acc, :k]), (k, mode, what)
    assert (data[~acc] == G_DATA).all(), (k, mode, what)                    # out_k untouched on a 0


@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("k", KS)
def test_full_error_range(gpu, orc, k, mode):
    t3 = gpu; B = rp.block_rows(k)
    rx, want, wok = expected(k, mode)
    n = len(rx)
    assert n > 20 * 256
    check(k, mode, slice(0, n), run_dev(t3, k, mode, rx), "all")
    mod_refused = np.flatnonzero((want != rx).any(axis=1) & (wok == 0))
    if mode == 0 and k <= 20:
        assert len(mod_refused) >= 20                                        # the partially modified rows went through the kernel
    # 255, 256, 257 blocks: across the near | far boundary, where accepted and refused rows meet
    for cnt in (255, 256, 257):
        rows = slice(B["far"].start - 100, B["far"].start - 100 + cnt)
        check(k, mode, rows, run_dev(t3, k, mode, rx[rows]), cnt)
    # the host-buffer form: ~1000 rows of every kind, data_k preset to the guard pattern
    pick = np.concatenate([np.arange(B["sched"].start, B["sched"].start + 300), np.arange(B["near"].start, B["near"].start + 200),
                           np.arange(B["far"].start, B["far"].start + 400), mod_refused[:100]])
    code = np.ascontiguousarray(rx[pick]).copy(); data = np.full((len(pick), k), G_DATA, np.uint8); ok = np.full(len(pick), G_OK, np.uint8)
    fn = t3.lib().t3hip_rs_decode_blocks
    fn.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    assert fn(k, mode, code.ctypes.data, len(pick), data.ctypes.data, ok.ctypes.data) == 0
    check(k, mode, pick, (code, data, ok), "host")
