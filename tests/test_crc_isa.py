"""The CRC path's gfx950 code as built (hipcc cross-compiles without a GPU; read from the objects build() leaves under csrc/).

LLVM recognises the bit-serial CRC-32 loop (`r = (r & 1) ? 0xEDB88320 ^ (r >> 1) : r >> 1`, eight times per byte) and replaces it by
a lookup table of its own in global memory (`.crctable*`): every byte step then becomes a global load whose address depends on the
previous one.  That made the frame record kernel a chain of ~64 memory round trips (14 us per frame behind the decoder)."""
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ternary-image-codec_amd", "csrc")
BIN = "/opt/rocm/lib/llvm/bin"


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()


def code_object(obj, td):
    fat, co = os.path.join(td, "fat.bin"), os.path.join(td, os.path.basename(obj) + ".co")
    subprocess.run([BIN + "/llvm-objcopy", "--dump-section", ".hip_fatbin=" + fat, obj], check=True, capture_output=True)
    subprocess.run([BIN + "/clang-offload-bundler", "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                    "--input=" + fat, "--output=" + co], check=True, capture_output=True)
    return co


def symbols(co):
    out = subprocess.run([BIN + "/llvm-readelf", "-s", co], check=True, capture_output=True, text=True).stdout
    return [line.split()[-1] for line in out.splitlines() if line.strip() and line.split()[0].rstrip(":").isdigit()]


def kernel_text(co, mangled_prefix):
    """The instructions of the one kernel whose symbol starts with mangled_prefix, in program order."""
    out = subprocess.run([BIN + "/llvm-objdump", "-d", "--no-show-raw-insn", co], check=True, capture_output=True, text=True).stdout
    body, inside = [], False
    for line in out.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.*)>:$", line)
        if m:
            if inside:
                break
            inside = m.group(1).startswith(mangled_prefix)
            continue
        if inside and line.startswith("\t"):
            body.append(line.split("//")[0].strip())
    assert body, mangled_prefix
    return body


def test_crc_kernels_carry_no_compiler_crc_table(built):
    with tempfile.TemporaryDirectory() as td:
        for obj in ("t3_decode.o", "t3_crc_fp4.o"):           # frame_record_kernel and crc_chunks_kernel / crc_fp4_kernel
            syms = symbols(code_object(os.path.join(CSRC, obj), td))
            assert syms, obj
            assert not [s for s in syms if s.startswith(".crctable")], obj


def test_frame_record_kernel_is_one_load_and_fold(built):
    """Every global load of the record kernel is issued before its first wait on vector memory, so no load address can depend on
    an earlier load's result, and the kernel waits on memory at most twice to completion."""
    with tempfile.TemporaryDirectory() as td:
        body = kernel_text(code_object(os.path.join(CSRC, "t3_decode.o"), td), "_ZN2t319frame_record_kernel")
    loads = [i for i, s in enumerate(body) if s.startswith("global_load")]
    waits = [i for i, s in enumerate(body) if s.startswith("s_waitcnt") and "vmcnt" in s]
    assert loads and waits
    assert max(loads) < min(waits), "a global load is issued after the kernel has waited on an earlier one"
    assert sum(1 for s in body if s.startswith("s_waitcnt") and "vmcnt(0)" in s) <= 2
