"""crc_fp4_kernel's first instructions, in the gfx950 code as built (the mechanism of test_crc_isa.py).

Every workgroup of the CRC launch starts at once, so whatever a wave does in front of its first payload load is a stretch in which
the chip reads no payload: the kernel used to stage an operator table into LDS, wait at a barrier and load its nine matrix slices
first.  Now the payload loads come first and nothing waits at a barrier in front of the round loop."""
import ctypes as C
import os
import re
import tempfile

import pytest

from test_crc_isa import CSRC, code_object, kernel_text

KERNEL = "_ZN2t314crc_fp4_kernel"


class CrcMArgs(C.Structure):               # mirrors t3_crc.h (only the offsets matter here)
    _fields_ = [("data", C.c_void_p), ("n_bytes", C.c_uint64), ("n_rounds", C.c_uint32), ("rounds_per_wave", C.c_uint32),
                ("stride_waves", C.c_uint32), ("afb", C.c_void_p), ("afrag", C.c_void_p), ("zpow", C.c_void_p),
                ("dist_lo", C.c_void_p), ("dist_hi", C.c_void_p), ("last_mod", C.c_uint32), ("chunk_crc", C.c_void_p),
                ("sym_sum", C.c_void_p), ("partials", C.c_void_p), ("tail_len", C.c_uint32)]


TABLE_POINTERS = ("afb", "afrag", "zpow", "dist_lo", "dist_hi")


@pytest.fixture(scope="module")
def body():
    import __graft_entry__ as ge
    ge.build()
    with tempfile.TemporaryDirectory() as td:
        return kernel_text(code_object(os.path.join(CSRC, "t3_crc_fp4.o"), td), KERNEL)


def first(body, prefix):
    hits = [i for i, s in enumerate(body) if s.startswith(prefix)]
    assert hits, prefix
    return hits[0]


def test_no_barrier_in_front_of_the_round_loop(body):
    assert not [i for i, s in enumerate(body[: first(body, "v_mfma")]) if s.startswith("s_barrier")]


def test_payload_loads_come_first(body):
    """The first global_load_dwordx4 is a payload load, and every load of a slice or distance table follows it: no vector load of any
    kind stands in front of it, and the tables' pointers have not even been fetched from the kernel arguments at that point."""
    i0 = first(body, "global_load_dwordx4")
    assert not [s for s in body[:i0] if re.match(r"(global|buffer|flat|scratch)_load", s)], "a load in front of the first payload load"
    sloads = [(i, re.match(r"s_load_dword(x(\d+))? s\[?[\d:]+\]?, (s\[\d+:\d+\]), (0x[0-9a-f]+|\d+)", s)) for i, s in enumerate(body) if s.startswith("s_load_dword")]
    assert sloads and all(m for _, m in sloads), [body[i] for i, m in sloads if not m]
    kernarg = sloads[0][1].group(3)                                       # the first scalar load of a kernel reads its arguments
    table_bytes = set()
    for name in TABLE_POINTERS:
        off = getattr(CrcMArgs, name).offset
        table_bytes.update(range(off, off + 8))
    fetched_at = []
    for i, m in sloads:
        if m.group(3) != kernarg:
            continue
        off, n = int(m.group(4), 0), 4 * int(m.group(2) or 1)
        if table_bytes & set(range(off, off + n)):
            fetched_at.append(i)
    assert fetched_at, "no table pointer is ever read from the kernel arguments"
    assert min(fetched_at) > i0, "a table pointer is fetched in front of the first payload load: tell the loads apart another way"
    assert getattr(CrcMArgs, "data").offset == 0 and any(m.group(3) == kernarg and int(m.group(4), 0) == 0 for i, m in sloads if i < i0)
