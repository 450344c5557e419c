"""The decode side's planner (csrc/t3_dec_plan.cpp) without a device and without the library: tests/cpp/dec_plan_demo.cpp plans a fixed
list of cases -- the fused decoder for each single k as raw words, pixels, RGB and in its repair form, with a beacon stepped over and over
tile ranges; the one-launch UEP / 2-D decoder for the ten (ra, rb) with either group first; the two-kernel decoder for one to four k; the
window and repair plans of one frame and of a batch -- on frames of 0 words to 8K, and prints the return code, the kernel value and every
argument the planner sets.  tests/golden/dec_plan.json holds the same records from the planners as they stood in t3_api_decode.cpp and
t3_api_repair.cpp before they had a unit of their own (recipe: profiles/decoder_host/notes.md).  Every field is compared for equality."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ternary-image-codec_amd", "csrc")
E_ARG = -3


@pytest.fixture(scope="module")
def records(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("dec_plan") / "dec_plan_demo")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wno-unknown-pragmas", "-I" + CSRC, os.path.join(ROOT, "tests", "cpp", "dec_plan_demo.cpp"),
                    os.path.join(CSRC, "t3_dec_plan.cpp"), os.path.join(CSRC, "t3_host.cpp"), "-o", exe], check=True)
    return json.loads(subprocess.run([exe], check=True, capture_output=True, text=True).stdout)


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "dec_plan.json")) as f:
        return json.load(f)


def test_plans_match_the_recorded_ones(records, golden):
    """Case by case, in order, no case missing on either side; within a case every field equal (a plan found: the kernel value and the
    argument fields; none: the return code alone)."""
    assert [r["case"] for r in records] == [g["case"] for g in golden]
    assert len(golden) >= 150 and len({g["case"] for g in golden}) == len(golden)
    for r, g in zip(records, golden):
        assert r.keys() == g.keys(), r["case"]
        for key in g:
            assert r[key] == g[key], (r["case"], key, r[key], g[key])


def test_case_list_reaches_every_branch(golden):
    """What the list is there for, read from the recorded side."""
    kind = lambda name: [g for g in golden if g["case"].split()[0] == name]
    found = lambda name: [g for g in kind(name) if g["rc"] == 0]
    fused, uep, stream = found("fused"), found("uep"), found("stream")
    # fused: every kernel value but RGB with r alone varying is reached -- each r as words, pixels, RGB and repair (512 threads, no tickets,
    # no output stage: the LDS ends 16 bytes behind the queue); a beacon in every form; frames of no tile's worth up to several tiles
    assert {(g["r"], g["px"], g["rgb"]) for g in fused} == {(r, px, rgb) for r in (2, 4, 6, 8) for (px, rgb) in ((0, 0), (1, 0), (1, 1))}
    assert {(g["px"], g["rgb"]) for g in fused if g["bcn"]} == {(0, 0), (1, 0), (1, 1)}
    assert {g["bcn_pb"] for g in fused if g["bcn"]} == {17, 26, 575} and {g["bcn_slot"] for g in fused if g["bcn"]} == {0, 8}
    repair = [g for g in fused if " repair " in g["case"]]
    assert {g["r"] for g in repair} == {2, 4, 6, 8} and all(g["lds_bytes"] == g["o_off"] + 16 and not g["tickets"] and g["nb"] == 52 for g in repair)
    assert any(" w=64 " in g["case"] for g in repair)                                   # the repair form takes a 2-D frame, the decoder forms do not
    assert {0, 1, 2, 3} <= {g["n_tiles"] for g in fused} | {0} and any(g["n_tiles"] >= 7 for g in fused)
    ranges = [g for g in fused if not g["whole_frame"]]
    assert any(g["out_off"] == 0 and g["n_tiles"] == 1 for g in ranges) and any(g["out_off"] > 0 and g["n_tiles"] == 3 for g in ranges)
    assert any(g["n_units"] < 6 * 108 * 22 for g in ranges if g["out_off"] == 6 * 6 * 108 * 22)      # the last tile alone: what is left of the stream
    refused = [g for g in kind("fused") if g["rc"] == E_ARG]
    assert any(" words " in g["case"] for g in refused) and any("beacon range" in g["case"] for g in refused)
    assert any("lo=3 hi=3" in g["case"] for g in refused) and any("lo=5 hi=3" in g["case"] for g in refused) and any("lo=9 " in g["case"] for g in refused)
    assert {g["case"].split()[1] for g in kind("fused") if g["rc"] == 1} == {"k22", "luma"}          # 2-D, two k
    # UEP: the ten kernels, the group swap (group 0's bands do not start at band 0), 2-D on and off, chunks clamped to n_sym, refusals
    assert {(g["ra"], g["rb"]) for g in uep} == {(a, b) for a in (2, 4, 6, 8) for b in (2, 4, 6, 8) if a >= b}
    assert any(g["n_grp"] == 2 and g["grp"][0]["bands"][0] != 0 for g in uep) and any(g["n_grp"] == 2 and g["grp"][0]["bands"][0] == 0 for g in uep)
    assert {g["il_on"] for g in uep} == {0, 1} and {4, 64, 512} <= {g["il_w"] for g in uep if g["il_on"]}
    assert any(g["il_on"] and g["il_A"] == g["n_sym"] for g in uep) and any(g["il_on"] and g["il_A"] < g["n_sym"] for g in uep)
    no = {g["case"] for g in kind("uep") if g["rc"] == 1}
    assert any(" w=6 " in c for c in no) and any("three k" in c for c in no) and any("two=1" in c for c in no) and any("body=268435456" in c for c in no)
    assert any("body=268435455" in g["case"] for g in uep) and all(g["lds_bytes"] <= 42 * 1280 for g in uep)
    # two kernels: one to four k, words and pixels, the granule-wise permutation and the symbol-wise one
    assert {g["n_grp"] for g in stream} == {1, 2, 3, 4} and {g["to_pixels"] for g in stream} == {0, 1}
    assert {(g["e_il_on"], g["e_il_fast"]) for g in stream} == {(0, 0), (1, 0), (1, 1)}
    assert any(g["e_lds_bytes"] == g["e_o_off"] for g in stream) and any(g["e_lds_bytes"] > g["e_o_off"] for g in stream)
    # window plans: a range, no range, an empty window, a window behind the stream, refusals, the knob; batches either side of 2^31 tickets
    win = kind("window") + kind("frames_window")
    assert {g["tile_range"] for g in win if g["rc"] == 0} == {0, 1} and any(g["rc"] == E_ARG for g in win)
    assert any(g["tile_range"] and g["tile_lo"] == g["tile_hi"] and g["n_px"] == 0 for g in win) and any(g["tile_range"] and 0 < g["tile_lo"] < g["tile_hi"] < g["n_tiles"] for g in win)
    assert any("generic=1" in g["case"] and g["tile_range"] == 0 for g in win) and {g["one_launch"] for g in kind("frames_window")} == {0, 1}
    assert any(g["rc"] == E_ARG and "tickets" in g["case"] for g in kind("frames_window")) and any(g["one_launch"] and "tickets" in g["case"] for g in kind("frames_window"))
    # repair plans: both paths, the batch in one launch or not, beacon and a 2-D frame with rows of no whole dwords on the generic path
    rep = kind("repair")
    assert {(g["path"], g["f_one_launch"]) for g in rep if g["rc"] == 0} == {(0, 0), (1, 0), (1, 1)} and any(g["rc"] == E_ARG for g in rep)
    by = {g["case"]: g for g in rep}
    assert by["repair k22 2d w=6 n=8192 frames=2"]["path"] == 0 and by["repair k22 2d w=4 n=8192 frames=2"]["path"] == 1
    assert by["repair k22 beacon w=0 n=8192 frames=3"]["path"] == 0 and all(g["blocks_per_tile"] == (468 if g["path"] else 256) for g in rep if g["rc"] == 0)
