"""stage_decode_kernel (t3hip_demap_rsdecode_bands[_dev]) across its workgroup steps: the lattice of tests/stage_shapes.py -- bodies of
63 .. 193 blocks per band, every beacon, code set and 16-byte phase in and out (tests/test_stage_shapes_lattice.py proves the lattice
reaches every edge) --, failures planted in several bands and workgroups at once, and one ~1.3 MB body whose bands carry the whole <= t
schedule of their code, where the expected output is a closed form of each arithmetic and no decoder.  Every comparison is bit-exact."""
import numpy as np
import pytest

import rs_patterns as rp
import stage_shapes as ss

pytestmark = pytest.mark.gpu
GUARD_IN, GUARD_OUT, PAD = 0x5C, 0xAB, 48


def run_dev(t3, body, hdr, code_k, code_mode, in_off, out_off):
    """-> (n_valid, the output): guards around the output intact, the input buffer byte-identical after the launch."""
    import torch
    n = len(body)
    total = t3.demap_rsdecode_bands_syms(n, hdr, code_k)
    buf = np.full(in_off + 9 * n + PAD, GUARD_IN, np.uint8); buf[in_off: in_off + 9 * n] = np.asarray(body, np.uint8).reshape(-1)
    d_in = torch.from_numpy(buf.copy()).cuda()
    d_out = torch.full((out_off + total + PAD,), GUARD_OUT, dtype=torch.uint8, device="cuda")
    d_nv = torch.zeros(1, dtype=torch.int64, device="cuda")
    assert d_in.data_ptr() % 16 == 0 and d_out.data_ptr() % 16 == 0        # the phases are the offsets' (test_stage_shapes_lattice.py)
    got_total = t3.demap_rsdecode_bands_dev(d_in.data_ptr() + in_off, n, hdr, code_k, code_mode, d_out.data_ptr() + out_off, total, d_nv.data_ptr(),
                                            torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert got_total == total
    assert (out[:out_off] == GUARD_OUT).all() and (out[out_off + total:] == GUARD_OUT).all()
    assert np.array_equal(d_in.cpu().numpy(), buf)                          # d_body9 is const
    return int(d_nv.item()), out[out_off: out_off + total]


@pytest.mark.parametrize("nb", ss.NBS)
def test_lattice(gpu, orc, nb):
    t3 = gpu
    for c in ss.lattice():
        if c["nb"] != nb:
            continue
        hdr, code_k, code_mode, body = ss.case_body(orc, t3.make_cfg, c)
        ok, want = ss.restate_stage3(orc, body, hdr, code_k, code_mode)
        nv, got = run_dev(t3, body, hdr, code_k, code_mode, c["in_off"], c["out_off"])
        assert len(got) == ss.case_geometry(c)["total"], c
        assert (nv == len(got)) == ok and nv == len(want), (c, nv, len(want))
        assert np.array_equal(got[:nv], want), c
        if c["i"] % 7 == 0:                                                 # the host-buffer form
            ok2, syms = t3.demap_rsdecode_bands(body, hdr, code_k, code_mode)
            assert ok2 == ok and np.array_equal(syms, want), c


@pytest.mark.parametrize("codeset", range(3))
def test_planted_failures(gpu, orc, codeset):
    """Blocks the band's own decoder refuses, in several bands and workgroups at once: n_valid is the band-major first of them."""
    t3 = gpu
    code_k, code_mode = ss.CODESETS[codeset]
    rng = np.random.default_rng([20261023, codeset])
    hdr = t3.make_cfg(uep=ss.PLANT_UEP, beacon=ss.PLANT_BEACON)
    geo = ss.geometry(ss.PLANT_WORDS, ss.PLANT_UEP, ss.PLANT_BEACON, code_k)
    clean = ss.stage_body(orc, rng, hdr, code_k, code_mode, ss.PLANT_WORDS, 0)
    for name, where in ss.plant_sets(geo["blocks"]).items():
        body = clean.copy()
        for b, m in where:
            ss.plant(body, hdr, b, m, ss.refused_row(orc, rng, geo["k"][b], code_mode[ss.PLANT_UEP[b] % 4]))
        first = min(geo["off"][b] + m * geo["k"][b] for b, m in where)
        ok, want = ss.restate_stage3(orc, body, hdr, code_k, code_mode)
        assert not ok and len(want) == first < geo["total"], name
        for j, off in enumerate(ss.PLANT_OFFS):
            nv, got = run_dev(t3, body, hdr, code_k, code_mode, ss.PLANT_OFFS[-1 - j], off)
            assert nv == first, (name, off, nv, first)
            assert np.array_equal(got[:nv], want), (name, off)
        ok2, syms = t3.demap_rsdecode_bands(body, hdr, code_k, code_mode)    # T3_E_RS with that prefix
        assert not ok2 and np.array_equal(syms, want), name


@pytest.fixture(scope="module")
def sched(orc, gpu):
    return ss.schedule_body(orc, gpu.make_cfg)


def test_schedule_fixed(gpu, orc, sched):
    """Every <= t pattern of every code, ~90 workgroups, beacon in slot 8: the original data, no oracle involved."""
    want = np.concatenate([d.reshape(-1) for d in sched["data"]])
    nv, got = run_dev(gpu, sched["body"], sched["hdr"], ss.KS, (1, 1, 1, 1), 5, 11)
    assert nv == len(want) == sched["geo"]["total"] and np.array_equal(got, want)


def test_schedule_compat(gpu, orc, sched):
    """The same body in COMPAT arithmetic: every block accepted, (cw + 2e)[:k] per block."""
    F = rp.field(orc); geo = sched["geo"]
    want = np.concatenate([F.add[sched["rx"][b], sched["e"][b]][:, : geo["k"][b]].reshape(-1) for b in range(9)])
    nv, got = run_dev(gpu, sched["body"], sched["hdr"], ss.KS, (0, 0, 0, 0), 9, 2)
    assert nv == len(want) == geo["total"] and np.array_equal(got, want)


def test_schedule_far_rows(gpu, orc, sched):
    """Far rows at two blocks per band, FIXED arithmetic: n_valid is the first of them, the prefix is the original data."""
    F = rp.field(orc); geo = sched["geo"]; hdr = sched["hdr"]
    body = sched["body"].copy()
    where = ss.schedule_far_blocks(geo)
    for i, (b, m) in enumerate(where):
        k = geo["k"][b]
        cw = F.sub[sched["rx"][b][m], sched["e"][b][m]]
        ss.plant(body, hdr, b, m, F.add[cw, rp.far_errors(k)[(i % 2) * 52 + i // 2]])     # per band an (s, 0, .., 0) row, then a pool row
    first = min(geo["off"][b] + m * geo["k"][b] for b, m in where)
    want = np.concatenate([d.reshape(-1) for d in sched["data"]])[:first]
    nv, got = run_dev(gpu, body, hdr, ss.KS, (1, 1, 1, 1), 0, 13)
    assert nv == first and np.array_equal(got[:nv], want)
    ok, syms = gpu.demap_rsdecode_bands(body, hdr, ss.KS, (1, 1, 1, 1))
    assert not ok and np.array_equal(syms, want)
