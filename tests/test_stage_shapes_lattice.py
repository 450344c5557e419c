"""The lattice of tests/stage_shapes.py reaches every edge stage_decode_kernel has (no GPU).  The edges come from the geometry of
plan_stages (t3_api_stages.cpp), restated in stage_shapes.geometry and held here to the columns the restatement builds: runs of 64 blocks
per band, a beacon band that ends in an earlier workgroup than the others, the 16-byte phase of the staged input run and of every wave's
output, mixed k and mixed arithmetic in one body.  The bodies are also held to closed forms: a clean body decodes to its data in both
arithmetics, and the schedule body to its data (FIXED) and to (cw + 2e)[:k] (COMPAT)."""
import numpy as np
import pytest

import oracle_lib as ol
import rs_patterns as rp
import stage_shapes as ss

CASES = ss.lattice()
GEO = [ss.case_geometry(c) for c in CASES]


def modes_of(c):
    code_mode = ss.CODESETS[c["codeset"]][1]
    return [code_mode[q % 4] for q in ss.UEPS[c["uep"]]]


def test_geometry_matches_the_columns():
    for c, g in zip(CASES, GEO):
        hdr = ol.make_cfg(uep=ss.UEPS[c["uep"]], beacon=c["beacon"])
        code_k = ss.CODESETS[c["codeset"]][0]
        off, total = ss.band_offsets(c["n_words"], hdr, code_k)
        assert (off, total) == (g["off"], g["total"]), c
        assert [len(ss.band_words(c["n_words"], hdr, b)) // 26 for b in range(9)] == g["blocks"], c
        assert all(g["blocks"][b] == c["nb"] for b in range(9) if b != g["bcn_band"]), c


def test_lattice_size_and_axes():
    assert 140 <= len(CASES) <= 160
    assert {c["nb"] for c in CASES} == set(ss.NBS) and {c["n_words"] - 26 * c["nb"] for c in CASES} == set(ss.TAILS)
    assert {c["beacon"] for c in CASES} == set(ss.BEACONS)
    for axis, n in (("codeset", 5), ("uep", 3)):
        assert {c[axis] for c in CASES} == set(range(n))
    assert {(c["codeset"], c["uep"]) for c in CASES} == {(a, b) for a in range(5) for b in range(3)}
    assert {c["corrupt"] for c in CASES} == set(ss.CORRUPT)
    for nb in ss.NBS:                                                       # every size at every corruption level and in both arithmetics
        sub = [c for c in CASES if c["nb"] == nb]
        assert {c["corrupt"] for c in sub} == set(ss.CORRUPT) and {m for c in sub for m in modes_of(c)} == {0, 1}, nb


def test_workgroup_steps():
    blocks = {n for g in GEO for n in g["blocks"]}
    for step in (1, 2):
        assert ss.STEP * step in blocks and ss.STEP * step + 1 in blocks and ss.STEP * step - 1 in blocks
    assert 3 * ss.STEP + 1 in blocks                                        # a last workgroup with one block
    # the beacon wave leaves a workgroup the other waves still work in: its band a whole number of runs, nb not
    early = [(c, g) for c, g in zip(CASES, GEO) if g["bcn_band"] < 9 and g["blocks"][g["bcn_band"]] and g["blocks"][g["bcn_band"]] % ss.STEP == 0
             and c["nb"] % ss.STEP != 0]
    assert early
    assert any(c["nb"] == 129 and c["beacon"][0] == 2 and g["blocks"][g["bcn_band"]] == 64 for c, g in early)
    for r in ss.TAILS:                                                      # period 2, nb = 129: 64 blocks whatever the tail
        assert ss.geometry(26 * 129 + r, ss.UEPS[0], (2, 8, 1), ss.KS)["blocks"][8] == 64
    # a beacon band with fewer workgroups than the others, with the same number, and an empty one (period 1)
    wgs = lambda n: -(-n // ss.STEP)
    rel = {(wgs(g["blocks"][g["bcn_band"]]) < wgs(c["nb"]), g["blocks"][g["bcn_band"]] == 0) for c, g in zip(CASES, GEO) if g["bcn_band"] < 9}
    assert rel == {(True, False), (False, False), (True, True)}
    # the beacon band's last workgroup holds fewer blocks than the others' (its lanes leave while the other waves' lanes work)
    assert any(0 < g["blocks"][g["bcn_band"]] % ss.STEP < c["nb"] % ss.STEP for c, g in zip(CASES, GEO) if g["bcn_band"] < 9)


def test_beacon_slots_and_mixed_codes():
    for slot in (0, 8):
        hit = [g for c, g in zip(CASES, GEO) if g["bcn_band"] == slot and g["blocks"][slot] and len({g["k"][b] for b in range(9) if b != slot}) >= 2]
        assert hit, slot
    mid = [g for c, g in zip(CASES, GEO) if g["bcn_band"] == 4 and g["blocks"][4] and len(set(g["k"][:4])) >= 2 and len(set(g["k"][5:])) >= 2]
    assert mid
    assert any(set(g["k"]) == {24, 22, 20, 18} for g in GEO)               # all four k in one body
    assert any(set(modes_of(c)) == {0, 1} and len(set(g["k"])) >= 2 for c, g in zip(CASES, GEO))   # both arithmetics, mixed k
    assert any(set(modes_of(c)) == {0, 1} and g["bcn_band"] < 9 and g["blocks"][g["bcn_band"]] for c, g in zip(CASES, GEO))


def test_every_16_byte_phase():
    """Device allocations are 16-byte aligned (the GPU test asserts it), so the phases are the offsets'."""
    assert {c["in_off"] & 15 for c in CASES} == set(range(16))
    assert {(c["out_off"] + g["off"][0]) & 15 for c, g in zip(CASES, GEO)} == set(range(16))
    later = {(c["out_off"] + g["off"][b]) & 15 for c, g in zip(CASES, GEO) for b in range(1, 9) if g["blocks"][b]}
    assert later == set(range(16))
    both = {(c["in_off"] & 15, c["out_off"] & 15) for c in CASES}           # chosen independently: neither fixes the other
    assert len({i for i, _ in both}) == 16 and len({o for _, o in both}) == 16 and len(both) >= 100
    for c, g in zip(CASES, GEO):                                            # a band's phase is the same in every workgroup
        assert all((ss.STEP * k) % 16 == 0 for k in g["k"])
    # head and tail of a wave's output: lengths cnt * k with every phase leave heads 0..15 and tails 0..15
    heads, tails = set(), set()
    for c, g in zip(CASES, GEO):
        for b in range(9):
            n = g["blocks"][b]
            for m0 in range(0, n, ss.STEP):
                ln = min(ss.STEP, n - m0) * g["k"][b]
                ph = (c["out_off"] + g["off"][b] + m0 * g["k"][b]) & 15
                head = min((16 - ph) & 15, ln)
                heads.add(head); tails.add((ln - head) % 16)
    assert heads == set(range(16)) and tails == set(range(16))


def test_plant_sets():
    geo = ss.geometry(ss.PLANT_WORDS, ss.PLANT_UEP, ss.PLANT_BEACON, ss.KS)
    assert geo["bcn_band"] == 4 and geo["blocks"][0] == 129 and 64 < geo["blocks"][4] < 128
    sets = ss.plant_sets(geo["blocks"])
    assert len(sets) == 6
    first = {}
    for name, where in sets.items():
        assert all(0 <= m < geo["blocks"][b] for b, m in where) and len(set(where)) == len(where), name
        first[name] = min(geo["off"][b] + m * geo["k"][b] for b, m in where)
    a = sets["a_min_in_last_workgroup"]
    assert first["a_min_in_last_workgroup"] == geo["off"][0] + 128 * geo["k"][0] and a[0][1] // ss.STEP == 2 > a[1][1] // ss.STEP
    b = sets["b_same_band_two_workgroups"]
    assert b[0][0] == b[1][0] and b[0][1] // ss.STEP != b[1][1] // ss.STEP and first["b_same_band_two_workgroups"] == geo["off"][2] + 5 * geo["k"][2]
    c = sets["c_beacon_wave_twice_and_later_band"]
    assert c[0][0] == c[1][0] == 4 and c[0][1] // ss.STEP == c[1][1] // ss.STEP and c[2][0] > 4
    assert first["d_first_block"] == 0
    assert first["e_last_block_of_last_band"] == geo["total"] - geo["k"][8]
    assert sorted(b for b, _ in sets["f_every_band"]) == list(range(9))


@pytest.mark.parametrize("nb", ss.NBS)
def test_clean_bodies_decode_to_their_data(orc, nb):
    """restate_stage3 on the clean bodies of the lattice: FIXED and COMPAT both return the data the body was built from."""
    for c in CASES:
        if c["nb"] != nb or c["corrupt"]:
            continue
        hdr, code_k, code_mode, body = ss.case_body(orc, ol.make_cfg, c)
        g = ss.case_geometry(c)
        want = np.concatenate([col[: 26 * g["blocks"][b]].reshape(-1, 26)[:, : g["k"][b]].reshape(-1) for b, col in enumerate(ss.band_columns(body, hdr))])
        assert len(want) == g["total"]
        for modes in (code_mode, (0, 0, 0, 0), (1, 1, 1, 1)):
            ok, got = ss.restate_stage3(orc, body, hdr, code_k, modes)
            assert ok and np.array_equal(got, want), (c, modes)


def test_schedule_body_closed_forms(orc):
    S = ss.schedule_body(orc, ol.make_cfg); geo = S["geo"]; F = rp.field(orc)
    assert geo["blocks"][0] == rp.schedule_len(18) + 2 and geo["bcn_band"] == 8 and geo["blocks"][8] < geo["blocks"][0]
    assert -(-geo["blocks"][0] // ss.STEP) >= 85 and 9 * ss.SCHED_WORDS < 1_400_000
    assert all(geo["blocks"][b] >= rp.schedule_len(geo["k"][b]) for b in range(9)) and set(geo["k"]) == {24, 22, 20, 18}
    data = np.concatenate([d.reshape(-1) for d in S["data"]])
    ok, got = ss.restate_stage3(orc, S["body"], S["hdr"], ss.KS, (1, 1, 1, 1))
    assert ok and np.array_equal(got, data)
    compat = np.concatenate([F.add[S["rx"][b], S["e"][b]][:, : geo["k"][b]].reshape(-1) for b in range(9)])
    ok, got = ss.restate_stage3(orc, S["body"], S["hdr"], ss.KS, (0, 0, 0, 0))
    assert ok and np.array_equal(got, compat) and not np.array_equal(compat, data)
    where = ss.schedule_far_blocks(geo)
    assert len(set(where)) == 18 and all(0 <= m < geo["blocks"][b] for b, m in where)
    assert min(geo["off"][b] + m * geo["k"][b] for b, m in where) == geo["off"][where[0][0]] + where[0][1] * geo["k"][where[0][0]]
