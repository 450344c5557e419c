"""Repair of a damaged 8K FIXED RS(26,20) frame in place against the only other route to a clean stream: decode to pixels and encode
again (profiles/repair/notes.md).  The frame carries the bench workload's 0..3 symbol errors per block.
    python3 profiles/repair_time.py                    the whole measurement: A B A B A B, then B on a clean frame and B as a dry run,
                                                       every side in a process of its own
    python3 profiles/repair_time.py --side A           one side: one JSON line
A      = t3hip_decode_frame_async (pixels) + t3hip_encode_frame_dev into a second coded buffer, on the build T3HIP_LIB_A names (the parent's
         libt3hip.so; this tree's when unset).
B      = t3hip_repair_frame_async with T3_REPAIR_WRITE on this tree's build.   Bclean: the same on the clean frame.   Bdry: B without the flag.
Every repetition works on a fresh copy of the frame: a device-to-device copy from a pristine buffer in front of the repetition's first
event (B repairs in place: without it every repetition but the first would see a clean frame).  Events without the system fence
(t3hip_event_*), one pair per repetition, 100 warm and 200 timed repetitions; mean, minimum and maximum per repetition in microseconds.
--reps / --warm: other counts (a kernel-trace run wants few)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FW, FH = 7680, 4320
SIDES = ("A", "B", "Bclean", "Bdry")


def one_side(side, warm, reps):
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch
    import __graft_entry__ as g
    import oracle_lib as ol
    t3 = g.load_package(); t3.init(0)
    n_px = FW * FH; n_raw = n_px // 2
    cfg = t3.make_cfg(profile=t3.ProfileID.P3_RS26_20, uep=2, mode=t3.MODE_FIXED)
    words = t3.encoded_words(n_raw, cfg); L = t3.plan(n_raw, cfg)
    s = torch.cuda.current_stream().cuda_stream
    d_px = torch.from_numpy(ol.oracle().lcg_pixels(n_px, 12345).view(np.uint8)).cuda()
    clean = torch.zeros(9 * words + 64, dtype=torch.uint8, device="cuda")
    t3.encode_frame_dev(d_px.data_ptr(), n_px, cfg, clean.data_ptr(), words, s)
    torch.cuda.synchronize()
    pristine = clean.clone()
    if side != "Bclean":
        t3.inject_errors_dev(pristine.data_ptr(), L.header_syms, L.body_syms // 26, 4242, 3, s)
    work = torch.zeros_like(pristine)
    ver = torch.zeros(4, dtype=torch.int32, device="cuda")
    W, V = work.data_ptr(), ver.data_ptr()
    if side == "A":
        d_out = torch.zeros(6 * n_px + 64, dtype=torch.uint8, device="cuda"); again = torch.zeros_like(pristine)
        O, E = d_out.data_ptr(), again.data_ptr()
        def op():
            t3.decode_frame_async(W, words, cfg, n_raw, O, n_px, V, True, s)
            t3.encode_frame_dev(O, n_px, cfg, E, words, s)
    else:
        flags = 0 if side == "Bdry" else t3.REPAIR_WRITE
        def op(): t3.repair_frame_async(W, words, cfg, n_raw, flags, V, s)
    res = {"side": side, "lib": "T3HIP_LIB (another build)" if os.environ.get("T3HIP_LIB") else "this tree", "warm": warm, "reps": reps}
    for _ in range(warm):
        work.copy_(pristine); op()
    torch.cuda.synchronize()
    ev = [(t3.Event(), t3.Event()) for _ in range(reps)]
    for e0, e1 in ev:
        work.copy_(pristine)                                   # outside the timed events
        e0.record(s); op(); e1.record(s)
    torch.cuda.synchronize()
    us = [1000.0 * e0.elapsed_ms(e1) for e0, e1 in ev]
    res["us_mean"], res["us_min"], res["us_max"] = round(sum(us) / len(us), 2), round(min(us), 2), round(max(us), 2)
    res["verdict"] = ver.cpu().tolist()
    out = again if side == "A" else work
    res["equals_clean"] = bool(torch.equal(out[: 9 * words], clean[: 9 * words]))      # A, B: the clean stream is back; Bdry: it is not
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", choices=SIDES)
    ap.add_argument("--warm", type=int, default=100); ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if a.side:
        return one_side(a.side, a.warm, a.reps)
    lib_a = os.environ.get("T3HIP_LIB_A")
    for side in ["A", "B"] * a.rounds + ["Bclean", "Bdry"]:
        env = dict(os.environ)
        env.pop("T3HIP_LIB", None)
        if side == "A" and lib_a: env["T3HIP_LIB"] = lib_a
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--side", side, "--warm", str(a.warm), "--reps", str(a.reps)],
                           env=env, capture_output=True, text=True, timeout=280)
        if r.returncode != 0:                                    # a side that failed ends the measurement: nothing more is started on the device
            sys.exit("repair_time: side %s failed (%d)\n%s" % (side, r.returncode, (r.stdout + r.stderr)[-3000:]))
        print(r.stdout.strip().splitlines()[-1], flush=True)


if __name__ == "__main__":
    main()
