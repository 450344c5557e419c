"""The strided FP4 CRC kernel's distance to the stream's end by table, against zlib.crc32.

A wave's remainder stands `lo + 2048 hi` bytes before the end of the stream: lo = the rest behind the last whole 2 KiB round, hi = the
rounds behind the wave's last one.  The kernel applies one operator from each of two tables ("append n bytes", "append 2048 n
bytes"), one column per lane, loaded at kernel entry.  With W waves striding over n_rounds rounds, wave g has
hi = ((n_rounds - 1) mod W - g) mod W: every stream has waves with hi = 0, 1 and W - 1, and n_rounds mod W decides which waves
wrap.  hi = W cannot be reached through the entry points (it would be a wave without a round, and every planned stride gives
every wave at least four rounds); the table's entry W exists so that the index is in bounds for any W.

W is taken from the device's CU count the way plan_crc takes it.  Every stream is a prefix of one random buffer, so the bytes behind a
stream's end are random too: a kernel that read past the end would change the result."""
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BENCH_WORDS = 20766726                     # one coded 8K frame (bench.py): 186,900,534 bytes
LEVELS = 8                                 # kCrcStrideLevels (t3_api_record.cpp)
LOS = (0, 1, 2047)
MODS = ("0", "1", "W-1")                   # (n_rounds - 1) mod W


def stride_w(slots, level):
    return max(4, (slots >> level) & ~3)


def planned_w(slots, n_rounds):
    """plan_crc: halve W until a wave has at least 8 rounds."""
    level = 0
    while level + 1 < LEVELS and stride_w(slots, level) * 8 > n_rounds:
        level += 1
    return stride_w(slots, level)


@pytest.fixture(scope="module")
def slots(gpu):
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count * 4 * 2


@pytest.fixture(scope="module")
def stream(gpu):
    import torch
    rng = np.random.default_rng(23)
    host = rng.integers(0, 27, size=9 * BENCH_WORDS + 4096, dtype=np.uint8)
    return host, torch.from_numpy(host).cuda()


_want = {}


def want_crc(host, n_bytes):
    if n_bytes not in _want:
        _want[n_bytes] = zlib.crc32(host[:n_bytes])
    return _want[n_bytes]


def rounds_for(slots, level, mod):
    """A round count that plan_crc gives stride level `level` and whose last round falls on wave `mod` of the stride."""
    w = stride_w(slots, level)
    lo_r = max(8 * w, 64) if level + 1 < LEVELS else 64                # the last level takes everything down to the threshold
    hi_r = 8 * stride_w(slots, level - 1) if level else 1 << 30
    m = {"0": 0, "1": 1 % w, "W-1": w - 1}[mod]
    n = lo_r + ((m + 1 - lo_r) % w)                                     # (n - 1) mod w == m
    if n < 64:
        n += w
    assert lo_r <= n < hi_r and (n - 1) % w == m and planned_w(slots, n) == w, (level, mod, n, w)
    return n, w


def check_record(gpu, orc, host, dev, n_words, scratch_bytes):
    import torch
    n_bytes = 9 * n_words
    rec = torch.zeros(gpu.FRAME_RECORD_BYTES, dtype=torch.uint8, device="cuda")
    scr = torch.full((scratch_bytes,), 0xA5, dtype=torch.uint8, device="cuda")
    gpu.frame_record_dev(dev.data_ptr(), n_words, 5, gpu.make_cfg(profile=2, uep=2), rec.data_ptr(), scr.data_ptr(), scratch_bytes)
    torch.cuda.synchronize()
    r = gpu.index_assemble(rec.cpu().numpy(), 0)[0]
    assert (r.frame_idx, r.n_words) == (5, n_words)
    print("record n_words %d scratch %d crc %08x want %08x" % (n_words, scratch_bytes, r.crc32, want_crc(host, n_bytes)))
    assert r.crc32 == want_crc(host, n_bytes), (n_words, scratch_bytes)
    assert r.sym_sum == orc.sym_sum(host[:n_bytes]), (n_words, scratch_bytes)


def words_near(slots, level, lo):
    """A word count whose 9 n bytes are a whole number of rounds of stride level `level` plus lo bytes."""
    rounds, w = rounds_for(slots, level, "1")
    base = 2048 * rounds // 9
    for k in range(64):                                                 # 9 n = lo (mod 2048) fixes n mod 2048; the round count then moves in steps of 9
        n = base + ((lo * pow(9, -1, 2048) - base) % 2048) + 2048 * k
        if (9 * n) % 2048 == lo and planned_w(slots, (9 * n) >> 11) == w:
            return n, w
    raise AssertionError((level, lo))


@pytest.mark.parametrize("level", range(LEVELS))
@pytest.mark.parametrize("mod", MODS)
def test_crc32_dev_distance(gpu, stream, slots, level, mod):
    host, dev = stream
    rounds, w = rounds_for(slots, level, mod)
    for lo in LOS:
        n_bytes = 2048 * rounds + lo
        got = gpu.crc32_dev(dev.data_ptr(), n_bytes)
        print("crc32_dev level %d W %d rounds %d lo %d: %08x want %08x" % (level, w, rounds, lo, got, want_crc(host, n_bytes)))
        assert got == want_crc(host, n_bytes), (level, w, rounds, lo)


@pytest.mark.parametrize("atomics", [False, True])
@pytest.mark.parametrize("level", range(LEVELS))
def test_frame_record_distance(gpu, orc, stream, slots, level, atomics, monkeypatch):
    """Partials (the record kernel folds them) and the accumulators with atomics: by the knob, and by a scratch without room."""
    if atomics:
        monkeypatch.setenv("T3HIP_CRC_ATOMICS", "1")
    host, dev = stream
    for lo in LOS:
        n, _ = words_near(slots, level, lo)
        check_record(gpu, orc, host, dev, n, gpu.frame_record_scratch_bytes(n))
        if not atomics:
            check_record(gpu, orc, host, dev, n, 64)


@pytest.mark.parametrize("atomics", [False, True])
def test_just_above_the_threshold(gpu, orc, stream, atomics, monkeypatch):
    """64 rounds is the shortest stream the matrix-core kernel takes: the narrowest stride, four rounds per wave."""
    if atomics:
        monkeypatch.setenv("T3HIP_CRC_ATOMICS", "1")
    host, dev = stream
    for rounds in (64, 65, 67, 79, 80):
        for lo in LOS + (9, 1026):
            n_bytes = 2048 * rounds + lo
            assert gpu.crc32_dev(dev.data_ptr(), n_bytes) == want_crc(host, n_bytes), (rounds, lo)
            if n_bytes % 9 == 0:
                check_record(gpu, orc, host, dev, n_bytes // 9, gpu.frame_record_scratch_bytes(n_bytes // 9))
    below = 64 * 2048 - 1                                               # (the table kernel's stream, for the boundary's other side)
    assert gpu.crc32_dev(dev.data_ptr(), below) == want_crc(host, below)


@pytest.mark.parametrize("atomics", [False, True])
def test_bench_payload(gpu, orc, stream, atomics, monkeypatch):
    if atomics:
        monkeypatch.setenv("T3HIP_CRC_ATOMICS", "1")
    host, dev = stream
    assert 9 * BENCH_WORDS == 186900534
    assert gpu.crc32_dev(dev.data_ptr(), 9 * BENCH_WORDS) == want_crc(host, 9 * BENCH_WORDS)
    check_record(gpu, orc, host, dev, BENCH_WORDS, gpu.frame_record_scratch_bytes(BENCH_WORDS))
    check_record(gpu, orc, host, dev, BENCH_WORDS, 64)
