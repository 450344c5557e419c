"""Repair of a batch of 16 equal damaged FIXED RS(26,20) frames in place: ONE t3hip_repair_frames_async call against a loop of
t3hip_repair_frame_async over the frames (profiles/repair_frames/notes.md).
    python3 profiles/repair_frames_time.py             the whole measurement: A B A B A B, every side in a process of its own; its
                                                       lines are kept as profiles/repair_frames/repair_frames_time.jsonl
    python3 profiles/repair_frames_time.py --side A    one side: one JSON line per workload
A = a loop of t3hip_repair_frame_async over the 16 frames, on the build T3HIP_LIB_A names (the parent's libt3hip.so; this tree's when
    unset).
B = one t3hip_repair_frames_async call on this tree's build.
Workloads: 16 frames of 1920 x 1080 and 16 of 1280 x 720, frame f at f * stride, stride = the frame's bytes rounded up to even; each as
`err` (the bench workload's 0..3 symbol errors per block, T3_REPAIR_WRITE), `clean` (clean frames, T3_REPAIR_WRITE) and `dry` (the
damaged frames without the flag).  Every repetition works on a fresh copy of the batch: a device-to-device copy from a pristine buffer in
front of the repetition's first event.  Events without the system fence (t3hip_event_*), one pair per repetition, 100 warm and 200
timed repetitions; mean, minimum and maximum per repetition in microseconds.  --reps / --warm: other counts (a kernel-trace run wants few)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_FRAMES = 16
SIZES = (("1080p", 1920, 1080), ("720p", 1280, 720))
VARIANTS = ("err", "clean", "dry")


def one_side(side, warm, reps):
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch
    import __graft_entry__ as g
    import oracle_lib as ol
    t3 = g.load_package(); t3.init(0)
    cfg = t3.make_cfg(profile=t3.ProfileID.P3_RS26_20, uep=2, mode=t3.MODE_FIXED)
    s = torch.cuda.current_stream().cuda_stream
    for label, fw, fh in SIZES:
        n_px = fw * fh; n_raw = n_px // 2
        words = t3.encoded_words(n_raw, cfg); L = t3.plan(n_raw, cfg)
        nb = 9 * words; stride = nb + (nb & 1)
        clean = torch.zeros(N_FRAMES * stride + 64, dtype=torch.uint8, device="cuda")
        one = torch.zeros(nb + 64, dtype=torch.uint8, device="cuda")
        for f in range(N_FRAMES):
            d_px = torch.from_numpy(ol.oracle().lcg_pixels(n_px, 12345 + f).view(np.uint8)).cuda()
            t3.encode_frame_dev(d_px.data_ptr(), n_px, cfg, one.data_ptr(), words, s)
            clean[f * stride: f * stride + nb].copy_(one[:nb])
        damaged = clean.clone()
        for f in range(N_FRAMES):
            one[:nb].copy_(damaged[f * stride: f * stride + nb])
            t3.inject_errors_dev(one.data_ptr(), L.header_syms, L.body_syms // 26, 4242 + f, 3, s)
            damaged[f * stride: f * stride + nb].copy_(one[:nb])
        torch.cuda.synchronize()
        work = torch.zeros_like(clean)
        ver = torch.zeros(4 * N_FRAMES, dtype=torch.int32, device="cuda")
        W, V = work.data_ptr(), ver.data_ptr()
        for variant in VARIANTS:
            pristine = clean if variant == "clean" else damaged
            flags = 0 if variant == "dry" else t3.REPAIR_WRITE
            if side == "A":
                def op():
                    for f in range(N_FRAMES):
                        t3.repair_frame_async(W + f * stride, words, cfg, n_raw, flags, V + 16 * f, s)
            else:
                def op(): t3.repair_frames_async(W, words, stride, N_FRAMES, cfg, n_raw, flags, V, s)
            res = {"side": side, "size": label, "variant": variant, "frames": N_FRAMES, "lib": "T3HIP_LIB (another build)" if os.environ.get("T3HIP_LIB") else "this tree",
                   "warm": warm, "reps": reps}
            for _ in range(warm):
                work.copy_(pristine); op()
            torch.cuda.synchronize()
            ev = [(t3.Event(), t3.Event()) for _ in range(reps)]
            for e0, e1 in ev:
                work.copy_(pristine)                               # outside the timed events
                e0.record(s); op(); e1.record(s)
            torch.cuda.synchronize()
            us = [1000.0 * e0.elapsed_ms(e1) for e0, e1 in ev]
            res["us_mean"], res["us_min"], res["us_max"] = round(sum(us) / len(us), 2), round(min(us), 2), round(max(us), 2)
            v = ver.cpu().numpy().reshape(N_FRAMES, 4)
            res["verdict_sum"] = [int(x) for x in v.sum(axis=0)]
            res["equals_clean"] = bool(torch.equal(work, clean))   # err, clean: the clean batch is back; dry: it is not
            print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", choices=("A", "B"))
    ap.add_argument("--warm", type=int, default=100); ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if a.side:
        return one_side(a.side, a.warm, a.reps)
    lib_a = os.environ.get("T3HIP_LIB_A")
    for side in ["A", "B"] * a.rounds:
        env = dict(os.environ)
        env.pop("T3HIP_LIB", None)
        if side == "A" and lib_a: env["T3HIP_LIB"] = lib_a
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--side", side, "--warm", str(a.warm), "--reps", str(a.reps)],
                           env=env, capture_output=True, text=True, timeout=280)
        if r.returncode != 0:                                        # a side that failed ends the measurement: nothing more is started on the device
            sys.exit("repair_frames_time: side %s failed (%d)\n%s" % (side, r.returncode, (r.stdout + r.stderr)[-3000:]))
        print("\n".join(l for l in r.stdout.strip().splitlines() if l.startswith("{")), flush=True)


if __name__ == "__main__":
    main()
