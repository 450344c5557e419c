"""CPU proof of the yardstick the repair tests hold the kernels to (tests/test_gpu_repair.py), and the host-only part of the repair
entries: the plan, the argument checks, the register budget of the fused kernel.

The repaired frame R' of a received FIXED frame R (include/t3hip.h, "repair"): a body block within t symbols of a codeword becomes that
codeword on the wire, canonical bytes 0..26, all 26 positions; any other block stays byte for byte as received; beacon slots and the
tail become what the encoder writes; the device entry never touches the header.

`expected(orc, fr, received)` builds R' from tests/rs_patterns.py and the oracle only.  The scrambler subtracts a state from every trit,
so what separates a received block (mod 27) from the clean block on the wire is the additive error row e itself (rs_patterns.apply), and
the clean block descrambles to a codeword c: the block lies within t of a codeword exactly when e alone does, and that codeword is
c + cw(e), cw(e) = what the oracle's block decoder returns for e alone -- added on the wire in the field.  Per case of rs_patterns:
  sched    Frame.clean
  near     clean plus, per placed row, cw(row), added with rs_patterns.apply
  far M    clean, except that the M blocks of `where` hold the received bytes
  lifted   the expected stream of the base (in a far block the lifted bytes stay)
Proven below: those four rows; the oracle's frame decoder gives the same answer -- pixels, verdict -- to `received` and to `expected`,
on the 2-D one-k frame as well (the blocks on the wire do not see the interleave); expected(expected) = expected; the verdict words
follow from (expected != received) and `where`."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as ol
import rs_patterns as rp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_HEADER, E_RS = -3, -5, -6
FUSED = rp.ONE_K + ("2d_64x64_k20",)                                     # path 1: one k on all bands, no beacon (1-D and 2-D)
GENERIC = ("k22_beacon2_slot8", "k20_beacon83", "luma", "four_codes", "2d_7x5_k22")
SWEEP = FUSED + GENERIC
SIZES = ("small", "padded", "full")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    return ge.load_package()


# ---- the yardstick ----------------------------------------------------------------------------------------------------------------------
def expected(orc, fr, received):
    """-> (R' flat, [uncorrectable blocks, blocks changed, bytes changed], sorted [(band, block)] of the uncorrectable blocks)"""
    F = rp.field(orc); L = fr.L
    rec = np.ascontiguousarray(received, np.uint8).reshape(-1)
    clean = fr.clean.reshape(-1)
    assert len(rec) == len(clean) == 9 * int(L.out_words)
    hs = int(L.header_syms)
    out = clean.copy()                                                    # beacon slots, tail: the encoder's bytes
    out[:hs] = rec[:hs]                                                   # the device entry never touches the header
    B = rp.block_index(L, fr.ocfg); f0 = rp.band_first_block(L)
    far = []
    for b in range(9):
        k, nb = fr.ks[b], fr.blocks[b]
        idx = B[f0[b]: f0[b] + nb]
        e = F.sub[rec[idx] % 27, clean[idx]]
        rows = np.flatnonzero(e.any(axis=1))
        if not len(rows):
            continue
        cw, _, ok = orc.rs_decode_blocks(k, e[rows], mode=1)
        good = ok == 1
        assert rp.is_codeword(orc, k, cw[good]).all() and ((cw[good] != e[rows[good]]).sum(axis=1) <= rp.tparam(k)).all()
        out[idx[rows[good]]] = F.add[clean[idx[rows[good]]], cw[good]]
        out[idx[rows[~good]]] = rec[idx[rows[~good]]]                     # byte for byte as received, bytes above 26 included
        far += [(b, int(m)) for m in rows[~good]]
    diff = out != rec
    words = [len(far), int(diff[B].any(axis=1).sum()), int(diff[hs:].sum())]
    return out, words, sorted(far)


def streams(fr, what):
    """(label, received, M, where, base label or None) for every stream of a frame at a size: rp.CASES, then rp.LIFTS on top of them"""
    for case in rp.CASES[what]:
        s, M, where = fr.stream(case)
        yield case, s, M, where, None
    for base, pattern in rp.lift_names(fr, what):
        s, _, M, where = rp.lifted(fr, base, pattern)
        yield "%s+%s" % (base, pattern), s, M, where, base


def _frame(built, orc, name, what):
    cfg = built.make_cfg(mode=1, **rp.CONFIGS[name])
    return rp.make_frame(orc, lambda n_raw: built.plan(n_raw, cfg), name, what)


def oracle_answer(orc, stream):
    rc, px = orc.decode_frame(np.ascontiguousarray(stream).reshape(-1, 9), ol.make_cfg(mode=1))
    return rc, px


@pytest.mark.parametrize("what", SIZES)
@pytest.mark.parametrize("name", SWEEP)
def test_expected_streams(built, orc, name, what):
    fr = _frame(built, orc, name, what)
    L = fr.L; clean = fr.clean.reshape(-1)
    B = rp.block_index(L, fr.ocfg); f0 = rp.band_first_block(L)
    by_label = {}
    for label, s, M, where, base in streams(fr, what):
        rec = s.reshape(-1)
        exp, words, far = expected(orc, fr, s)
        by_label[label] = exp
        tag = (name, what, label)
        far_rows = [f0[b] + m for (b, m) in where]
        assert far == sorted(where) and words[0] == M, tag
        # the table of the module docstring
        want = clean.copy()
        if label == "near":
            F = rp.field(orc); cwb = []; placed = 0
            for b in range(9):
                idx = B[f0[b]: f0[b] + fr.blocks[b]]
                e = F.sub[rec[idx], clean[idx]]
                rows = np.flatnonzero(e.any(axis=1)); placed += len(rows)
                z = np.zeros_like(e)
                if len(rows):
                    cw, _, ok = orc.rs_decode_blocks(fr.ks[b], e[rows], mode=1)
                    assert (ok == 1).all() and (cw != 0).any(axis=1).all(), tag         # within t of ANOTHER codeword
                    z[rows] = cw
                cwb.append(z)
            assert placed == sum(fr.near()[1].values()), tag
            want = rp.apply(orc, fr.clean, L, fr.ocfg, cwb).reshape(-1)
            assert not np.array_equal(want, clean), tag
        if base is not None and base != "clean":
            want = (by_label[base] if base in by_label else expected(orc, fr, fr.stream(base)[0])[0]).copy()   # lifted: the expected stream of the base ...
        want[B[far_rows].reshape(-1)] = rec[B[far_rows].reshape(-1)]                     # ... far blocks hold the received (lifted) bytes
        assert np.array_equal(exp, want), tag
        if M == 0 and label != "near":
            assert np.array_equal(exp, clean), tag
        # the words follow from (expected != received) and `where`
        diff = exp != rec
        assert not diff[: int(L.header_syms)].any() and not diff[B[far_rows]].any(), tag
        assert words == [M, int(diff[B].any(axis=1).sum()), int(diff.sum())], tag
        if base is None and label != "near" and M == 0:
            assert words[1] == int((rec[B] != clean[B]).any(axis=1).sum()) > 0, tag
        # a fixed point
        exp2, words2, far2 = expected(orc, fr, exp.reshape(-1, 9))
        assert np.array_equal(exp2, exp) and words2 == [M, 0, 0] and far2 == far, tag
        # the oracle's frame decoder: same verdict, same pixels
        a, b = oracle_answer(orc, s), oracle_answer(orc, exp)
        assert a[0] == b[0] == (E_RS if M else 0), tag
        if not M:
            assert np.array_equal(a[1], b[1]), tag
            if label != "near":
                assert np.array_equal(a[1], fr.padded), tag
    exp, words, _ = expected(orc, fr, fr.clean)
    assert np.array_equal(exp, clean) and words == [0, 0, 0]                             # a clean canonical frame: zero stores


# ---- the plan and the argument checks ---------------------------------------------------------------------------------------------------
def test_plan_over_configs(built):
    t3 = built
    for name, kw in rp.CONFIGS.items():
        cfg = t3.make_cfg(mode=1, **kw)
        for n_raw in (151, 40000):
            p = t3.repair_plan(n_raw, cfg); L = t3.plan(n_raw, cfg)
            assert p.path == (1 if name in FUSED else 0), (name, n_raw)
            assert p.in_bytes == 9 * int(L.out_words)
            blocks = [int(L.band_blocks[b]) for b in range(9)]
            if p.path:
                assert p.blocks_per_tile == 9 * 52 and p.n_tiles == -(-max(blocks) // 52)
            else:
                assert p.blocks_per_tile == 256 and p.n_tiles == -(-sum(blocks) // 256)
        for bad in (t3.make_cfg(mode=0, **kw), t3.make_cfg(mode=1, **dict(kw, profile=0xFF))):      # COMPAT, RAW mode
            with pytest.raises(t3.T3Error) as e:
                t3.repair_plan(40000, bad)
            assert e.value.code == E_ARG
    assert t3.repair_plan(0, t3.make_cfg(mode=1, profile=2, uep=2)).path == 0               # an empty frame: nothing for the fused kernel
    with pytest.raises(t3.T3Error) as e:                                                   # a FIXED limit: beacon slot >= 9
        t3.repair_plan(100, t3.make_cfg(mode=1, profile=2, uep=2, beacon=(4, 9, 1)))
    assert e.value.code == E_ARG


NODEV = r"""
import ctypes as C, sys
sys.path.insert(0, %r)
import __graft_entry__ as ge
t3 = ge.load_package()
L = t3.lib()
assert not t3.is_ready()
cfg = t3.make_cfg(profile=2, uep=2, mode=1); compat = t3.make_cfg(profile=2, uep=2, mode=0); raw = t3.make_cfg(profile=0xFF, mode=1)
n_raw = 64; n_in = int(t3.plan(n_raw, cfg).out_words)
buf = (C.c_uint8 * (9 * n_in + 16))(); ver = (C.c_uint32 * 4)(); cnt = (C.c_uint32 * 4)()
base = C.addressof(buf); base += base & 1
def run(io=base, n=n_in, c=cfg, flags=1, v=C.addressof(ver)):
    return L.t3hip_repair_frame_async(C.c_void_p(io), C.c_uint64(n), C.byref(c) if c is not None else None, C.c_uint64(n_raw), C.c_uint32(flags), C.c_void_p(v), None)
E_ARG, E_HEADER = -3, -5
assert run(c=None) == E_ARG and run(v=None) == E_ARG and run(io=None) == E_ARG and run(io=base + 1) == E_ARG and run(flags=2) == E_ARG
assert run(c=compat) == E_ARG and run(c=raw) == E_ARG
assert run(n=n_in - 1) == E_HEADER
assert run() == t3.E_NODEVICE and run(flags=0) == t3.E_NODEVICE and run(io=base + 2) == t3.E_NODEVICE
seen = t3.DecoderContext(mode=1).cfg_last_seen
assert L.t3hip_repair_profile_dev(C.c_void_p(base), C.c_uint64(n_in), C.byref(compat), C.c_uint32(1), cnt, None) == E_ARG
assert L.t3hip_repair_profile_dev(C.c_void_p(base), C.c_uint64(n_in), C.byref(seen), C.c_uint32(1), None, None) == E_ARG
assert L.t3hip_repair_profile_dev(C.c_void_p(base), C.c_uint64(n_in), C.byref(seen), C.c_uint32(1), cnt, None) == t3.E_NODEVICE
assert L.t3hip_repair_profile(C.c_void_p(base), C.c_uint64(n_in), C.byref(compat), C.c_uint32(1), cnt) == E_ARG
assert L.t3hip_repair_profile(C.c_void_p(base), C.c_uint64(n_in), C.byref(seen), C.c_uint32(1), cnt) == t3.E_NODEVICE
assert t3.repair_plan(n_raw, cfg).path == 1
print("ok")
"""


def test_arguments_then_the_device(built):
    """A process that never initialised a device: every bad argument is refused before the entries ask for one, and only then
    T3_E_NODEVICE (no CPU fallback); the plan answers.  (The addresses are host memory and never read: no device, no launch.)"""
    r = subprocess.run([sys.executable, "-c", NODEV % ROOT], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_fused_kernel_register_budget(built):
    """repair_fixed_kernel<R> for the four codes: built once each, no spilled VGPR, no scratch access inside the tile loop, 80 VGPRs at
    most (three 8-wave workgroups per CU); the generic kernel is there."""
    sys.path.insert(0, os.path.join(ROOT, "profiles"))
    import kernel_resources as kr
    ks = kr.all_kernels()
    loops = kr.loop_scratch(["t3_repair.o"])
    for r in (2, 4, 6, 8):
        hit = [n for n in ks if "repair_fixed_kernel<%d>" % r in n]
        assert len(hit) == 1, (r, hit)
        assert int(ks[hit[0]]["vgpr_spill_count"]) == 0 and int(ks[hit[0]]["vgpr_count"]) <= 80, (hit[0], ks[hit[0]])
        assert loops[hit[0]] == (0, 0), (hit[0], loops[hit[0]])
    assert len([n for n in ks if "repair_generic_kernel" in n]) == 1
