"""Per-kernel register / spill / LDS figures of the built library's gfx950 code objects (hipcc cross-compiles without a GPU):
    python3 profiles/kernel_resources.py [substring ...]
    python3 profiles/kernel_resources.py --diff OBJDIR_A OBJDIR_B [substring ...]
Reads the objects under ternary-image-codec_amd/csrc/*.o: .hip_fatbin -> clang-offload-bundler -> llvm-readelf --notes / llvm-objdump.
--diff compares two builds of the library (make OBJDIR=...) kernel by kernel: instruction mnemonics in order, and the resource lines.
Kernels are matched by demangled name over all objects of each directory, so the two builds may cut their translation units differently.
Used by tests/test_host_logic.py::test_no_vgpr_spills_in_hot_kernels and by hand while budgeting registers."""
import contextlib, os, re, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = "/opt/rocm/lib/llvm/bin"
CSRC = os.path.join(ROOT, "ternary-image-codec_amd", "csrc")


@contextlib.contextmanager
def code_object(obj, must=True):
    """The gfx950 code object inside a host object file, as a temporary file.  An object without device code, or a tool that fails:
    an error, or None with must=False (all_kernels walks host-only objects too)."""
    with tempfile.TemporaryDirectory() as td:
        fat, co = os.path.join(td, "fat.bin"), os.path.join(td, "k.co")
        r = subprocess.run([BIN + "/llvm-objcopy", "--dump-section", ".hip_fatbin=" + fat, obj], capture_output=True, check=must)
        if r.returncode or not os.path.exists(fat) or os.path.getsize(fat) == 0:
            if must:
                raise RuntimeError("no .hip_fatbin in " + obj)
            yield None
            return
        r = subprocess.run([BIN + "/clang-offload-bundler", "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + fat, "--output=" + co],
                           capture_output=True, check=must)
        yield None if r.returncode else co


def kernel_notes(obj):
    with code_object(obj, must=False) as co:
        if co is None:
            return {}
        txt = subprocess.run([BIN + "/llvm-readelf", "--notes", co], capture_output=True, text=True).stdout
    out, cur = {}, None
    for line in txt.splitlines():
        m = re.match(r"\s*-?\s*\.(\w+):\s*(.*)$", line)
        if not m:
            continue
        k, v = m.group(1), m.group(2).strip()
        if k == "agpr_count" or (k == "args"):
            cur = {} if k == "agpr_count" else cur
        if cur is None:
            cur = {}
        if k in ("name", "vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size"):
            cur[k] = v
        if k == "wavefront_size":                      # last key of a kernel record
            if "name" in cur:
                out[cur["name"]] = cur
            cur = None
    return out


def demangle(names):
    for tool in (BIN + "/llvm-cxxfilt", "c++filt"):
        try:
            r = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True)
            if r.returncode == 0 and len(r.stdout.splitlines()) == len(names):
                return dict(zip(names, r.stdout.splitlines()))
        except OSError:
            pass
    return {n: n for n in names}


def all_kernels():
    res = {}
    for f in sorted(os.listdir(CSRC)):
        if f.endswith(".o"):
            res.update(kernel_notes(os.path.join(CSRC, f)))
    dm = demangle(list(res))
    return {dm[k]: v for k, v in res.items()}


def resource_line(v):
    return "vgpr %3s spill %2s | sgpr %3s spill %2s | scratch %s | lds %s" % (v.get("vgpr_count"), v.get("vgpr_spill_count"), v.get("sgpr_count"), v.get("sgpr_spill_count"),
                                                                             v.get("private_segment_fixed_size"), v.get("group_segment_fixed_size"))


def disassembly(obj):
    """{mangled function: [(address, instruction text, comment tail), ...]} of an object's gfx950 code."""
    with code_object(obj) as co:
        txt = subprocess.run([BIN + "/llvm-objdump", "-d", "--no-show-raw-insn", co], capture_output=True, text=True, check=True).stdout
    cur, funcs = None, {}
    for line in txt.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
        if m:
            cur = m.group(1); funcs[cur] = []; continue
        m = re.match(r"^\s+(\S.*?)\s*//\s*([0-9A-Fa-f]+):(.*)$", line)
        if m and cur:
            funcs[cur].append((int(m.group(2), 16), m.group(1), m.group(3)))
    return {k: v for k, v in funcs.items() if v}


def mnemonic_list(body):
    return [text.split()[0] for _, text, _ in body]


def mnemonics(obj):
    """{kernel (demangled): [mnemonic, ...]} in program order (kernels only: the functions that have a resource record)."""
    funcs, notes = disassembly(obj), kernel_notes(obj)
    dm = demangle(list(funcs))
    return {dm[k]: mnemonic_list(body) for k, body in funcs.items() if k in notes}


def tile_loop(body):
    """The persistent tile loop of a kernel = the widest backward-branch range that holds a matrix instruction, as (first, last)
    instruction index; None for a kernel without one."""
    index = {addr: i for i, (addr, _, _) in enumerate(body)}
    loops = []
    for i, (addr, text, tail) in enumerate(body):
        if text.startswith("s_cbranch") or text.startswith("s_branch"):
            m = re.search(r"<\S+\+0x([0-9a-fA-F]+)>", tail)
            tgt = body[0][0] + int(m.group(1), 16) if m else None
            if tgt is not None and tgt <= addr and tgt in index:
                loops.append((index[tgt], i))
    mf = [i for i, (_, t, _) in enumerate(body) if "v_mfma" in t]
    best = None
    for lo, hi in loops:
        if any(lo <= i <= hi for i in mf) and (best is None or body[hi][0] - body[lo][0] > body[best[1]][0] - body[best[0]][0]):
            best = (lo, hi)
    return best


def device_objects(objdir=CSRC):
    """The object files of a directory, by name (those without device code yield no kernels)."""
    return [f for f in sorted(os.listdir(objdir)) if f.endswith(".o")]


def kernel_bodies(objdir, obj_names=None):
    """{kernel (demangled): (object file, disassembly, resource record)} over the objects of a directory (default: all of them)."""
    res = {}
    for f in obj_names or device_objects(objdir):
        p = os.path.join(objdir, f)
        notes = kernel_notes(p)
        if not notes:
            continue
        funcs = disassembly(p)
        dm = demangle(list(notes))
        for k, v in notes.items():
            if k in funcs:
                assert dm[k] not in res, "kernel in two objects: " + dm[k]
                res[dm[k]] = (f, funcs[k], v)
    return res


def loop_scratch(obj_names=None, objdir=CSRC):
    """Scratch (spill) accesses INSIDE the persistent tile loop of every kernel that has one: {kernel: (loads, stores)}, over every
    object that holds device code (or the named ones).
    (The reload of a spilled register is followed by s_waitcnt vmcnt(0), which also drains the next tile's prefetch -- profiles/r02/notes.md)."""
    res = {}
    for name, (_, body, _) in kernel_bodies(objdir, obj_names).items():
        best = tile_loop(body)
        if best is None:
            continue
        inside = [t for _, t, _ in body[best[0]: best[1] + 1]]
        res[name] = (sum(1 for t in inside if t.startswith("scratch_load")), sum(1 for t in inside if t.startswith("scratch_store")))
    return res


def diff(dir_a, dir_b, only=()):
    """Two builds of the library, kernel by kernel (matched by demangled name, whichever object holds it): are the mnemonic sequences
    equal (if not: the first differing index, and whether it lies inside the tile loop), and the two resource lines.  `only`: substrings
    of the kernel names to compare.  Returns the number of kernels that differ in either."""
    ka, kb = kernel_bodies(dir_a), kernel_bodies(dir_b)
    names = sorted(n for n in set(ka) | set(kb) if not only or any(s in n for s in only))
    print("== %d / %d kernels" % (sum(n in ka for n in names), sum(n in kb for n in names)))
    n_diff = 0
    for k in names:
        if k not in ka or k not in kb:
            n_diff += 1
            print("%s\n    only in %s" % (k, dir_a if k in ka else dir_b))
            continue
        (fa, da, na), (fb, db, nb) = ka[k], kb[k]
        ma, mb = mnemonic_list(da), mnemonic_list(db)
        ra, rb = resource_line(na), resource_line(nb)
        la, lb = tile_loop(da), tile_loop(db)
        sa = sum(1 for _, t, _ in (da[la[0]: la[1] + 1] if la else []) if t.startswith("scratch_"))
        sb = sum(1 for _, t, _ in (db[lb[0]: lb[1] + 1] if lb else []) if t.startswith("scratch_"))
        if ma == mb:
            verdict = "mnemonics equal (%d)" % len(ma)
        else:
            i = next((i for i, (x, y) in enumerate(zip(ma, mb)) if x != y), min(len(ma), len(mb)))
            where = "no tile loop" if la is None else "inside the tile loop" if la[0] <= i <= la[1] else "before the tile loop" if i < la[0] else "behind the tile loop"
            same_loop = la is not None and lb is not None and ma[la[0]: la[1] + 1] == mb[lb[0]: lb[1] + 1]
            verdict = "mnemonics DIFFER: %d vs %d instructions, first at index %d (%s vs %s), %s [%s]%s" % (
                len(ma), len(mb), i, ma[i] if i < len(ma) else "-", mb[i] if i < len(mb) else "-", where, "%d..%d" % la if la else "-",
                "" if la is None else "; tile loop itself " + ("equal" if same_loop else "DIFFERS"))
        if ma != mb or ra != rb or sa != sb:
            n_diff += 1
        print("%s  [%s | %s]\n    %s\n    A: %s | loop scratch %d\n    B: %s | loop scratch %d" % (k, fa, fb, verdict, ra, sa, rb, sb))
    print("kernels that differ: %d of %d" % (n_diff, len(names)))
    return n_diff


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--diff":
        if len(sys.argv) < 4:
            sys.exit(__doc__)
        sys.exit(1 if diff(sys.argv[2], sys.argv[3], tuple(sys.argv[4:])) else 0)
    ks = all_kernels()
    for name in sorted(ks):
        if len(sys.argv) > 1 and not any(s in name for s in sys.argv[1:]):
            continue
        print("%-90s %s" % (name[:90], resource_line(ks[name])))
