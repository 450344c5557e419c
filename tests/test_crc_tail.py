"""The rest behind the CRC kernel's whole 2 KiB rounds (fewer than 2048 bytes, taken by the FP4 kernel's first workgroup) and the
frame record's one load-and-fold, against zlib and the oracle's symbol sum.

Every stream is a prefix of one random buffer, so the bytes behind a stream's end are random too: a kernel that read past the
end would change the result."""
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BENCH_WORDS = 20766726                     # one coded 8K frame (bench.py): 186,900,534 bytes, a 54-byte rest
TAILS = (0, 1, 3, 4, 15, 16, 17, 54, 1023, 2047)
# 2 KiB rounds per stream: the FP4 kernel strides its rounds over every wave slot of the chip (2048 on 256 CUs) from 8 rounds per
# slot on, and over half of them below that
ROUNDS_FULL, ROUNDS_HALF = 20000, 10000
KNOBS = ("T3HIP_CRC_ATOMICS", "T3HIP_CRC_BLOCKED", "T3HIP_CRC_TABLES")


@pytest.fixture(scope="module")
def stream():
    import torch
    rng = np.random.default_rng(11)
    host = rng.integers(0, 27, size=9 * BENCH_WORDS + 4096, dtype=np.uint8)
    return host, torch.from_numpy(host).cuda()


def words_for(rounds, tail):
    """A word count n near `rounds` rounds with 9 n = 2048 m + tail."""
    base = 2048 * rounds // 9
    n = base + ((tail * pow(9, -1, 2048) - base) % 2048)
    assert (9 * n) % 2048 == tail
    return n


def check_record(gpu, orc, host, dev, n_words, scratch_bytes, misalign=False):
    import torch
    n_bytes = 9 * n_words
    rec = torch.zeros(gpu.FRAME_RECORD_BYTES, dtype=torch.uint8, device="cuda")
    scr = torch.full((scratch_bytes + 8,), 0xA5, dtype=torch.uint8, device="cuda")
    ptr = scr.data_ptr() + (4 if misalign else 0)          # (torch allocations are 512-byte aligned: +4 is 4- but not 8-byte aligned)
    assert ptr % 8 == (4 if misalign else 0)
    gpu.frame_record_dev(dev.data_ptr(), n_words, 3, gpu.make_cfg(profile=2, uep=2), rec.data_ptr(), ptr, scratch_bytes)
    torch.cuda.synchronize()
    r = gpu.index_assemble(rec.cpu().numpy(), 0)[0]
    payload = host[:n_bytes]
    assert (r.frame_idx, r.n_words) == (3, n_words)
    assert r.crc32 == zlib.crc32(payload), (n_words, scratch_bytes, misalign)
    assert r.sym_sum == orc.sym_sum(payload), (n_words, scratch_bytes, misalign)
    assert list(r.header_syms)[: min(54, n_bytes)] == list(payload[:54])


@pytest.mark.parametrize("rounds", [ROUNDS_FULL, ROUNDS_HALF])
@pytest.mark.parametrize("tail", TAILS)
def test_record_rest(gpu, orc, stream, rounds, tail):
    host, dev = stream
    n = words_for(rounds, tail)
    check_record(gpu, orc, host, dev, n, 64)
    check_record(gpu, orc, host, dev, n, gpu.frame_record_scratch_bytes(n), misalign=True)


@pytest.mark.parametrize("rounds", [ROUNDS_FULL, ROUNDS_HALF])
@pytest.mark.parametrize("tail", TAILS)
def test_crc32_dev_rest(gpu, stream, rounds, tail):
    host, dev = stream
    n_bytes = 2048 * rounds + tail
    assert gpu.crc32_dev(dev.data_ptr(), n_bytes) == zlib.crc32(host[:n_bytes]), n_bytes


def test_record_bench_frame(gpu, orc, stream):
    host, dev = stream
    check_record(gpu, orc, host, dev, BENCH_WORDS, 64)
    check_record(gpu, orc, host, dev, BENCH_WORDS, gpu.frame_record_scratch_bytes(BENCH_WORDS))
    check_record(gpu, orc, host, dev, BENCH_WORDS, gpu.frame_record_scratch_bytes(BENCH_WORDS), misalign=True)
    assert gpu.crc32_dev(dev.data_ptr(), 9 * BENCH_WORDS) == zlib.crc32(host[: 9 * BENCH_WORDS])


@pytest.mark.parametrize("knob", KNOBS)
def test_record_rest_knobs(gpu, orc, stream, knob, monkeypatch):
    """The measurement knobs still give correct records and CRCs (the table kernels leave the rest to crc_chunks_kernel)."""
    monkeypatch.setenv(knob, "1")
    host, dev = stream
    for tail in (0, 1, 54, 2047):
        n = words_for(ROUNDS_HALF, tail)
        for nscr in (64, gpu.frame_record_scratch_bytes(n)):
            check_record(gpu, orc, host, dev, n, nscr)
        n_bytes = 2048 * ROUNDS_HALF + tail
        assert gpu.crc32_dev(dev.data_ptr(), n_bytes) == zlib.crc32(host[:n_bytes]), (knob, n_bytes)
