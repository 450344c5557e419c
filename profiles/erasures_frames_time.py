"""Repair with erasures of a batch of equal FIXED RS(26,20) frames in place: ONE t3hip_repair_erasures_frames_async call against a loop
of t3hip_repair_erasures_frame_async over the frames, and against the plain batch (profiles/erasures_frames/notes.md).
    python3 profiles/erasures_frames_time.py             the whole measurement: A B C A B C A B C (A and B alternate), every side in a
                                                         process of its own; its lines are kept as
                                                         profiles/erasures_frames/erasures_frames_time.jsonl
    python3 profiles/erasures_frames_time.py --side A    one side: one JSON line per batch and workload
A = a loop of N t3hip_repair_erasures_frame_async calls, on the build T3HIP_LIB_A names (the parent's libt3hip.so; this tree's when unset).
B = one t3hip_repair_erasures_frames_async call on this tree's build.
C = one t3hip_repair_frames_async call (the plain batch) on the build T3HIP_LIB_A names, workloads `clean` and `err` only: what two
    workgroups per CU instead of three cost here.
All with T3_REPAIR_WRITE.  Batches: 16 frames of 854 x 480 and 8 frames of 1920 x 1080, frame f at f * stride, stride = the frame's bytes
rounded up to even.  The three workloads of profiles/erasures/notes.md section 2:
  clean   clean frames
  err     the bench workload's 0..3 trit errors per block (t3hip_inject_errors_dev, a seed per frame): no byte above 26
  bytes   byte corruption: per block 0..6 bytes replaced by uniform random bytes (erasures_time.corrupt_bytes, a seed per frame)
Every repetition works on a fresh copy of the batch: a device-to-device copy from a pristine buffer in front of the repetition's first
event.  Events without the system fence (t3hip_event_*), one pair per repetition, 100 warm and 200 timed repetitions; mean, minimum and
maximum per repetition in microseconds, the per-word sums of the frames' verdict words, and a hash of the batch after the last
repetition (A and B must agree in both)."""
import argparse
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCHES = (("480p", 854, 480, 16), ("1080p", 1920, 1080, 8))
SEED = 20261020


def one_side(side, warm, reps):
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "profiles"))
    import numpy as np
    import torch
    import __graft_entry__ as g
    import oracle_lib as ol
    from erasures_time import corrupt_bytes
    t3 = g.load_package(); t3.init(0)
    cfg = t3.make_cfg(profile=t3.ProfileID.P3_RS26_20, uep=2, mode=t3.MODE_FIXED)
    s = torch.cuda.current_stream().cuda_stream
    nw = 4 if side == "C" else 6
    for label, fw, fh, N in BATCHES:
        n_px = fw * fh; n_raw = n_px // 2
        words = t3.encoded_words(n_raw, cfg); L = t3.plan(n_raw, cfg)
        hs, nblk = int(L.header_syms), int(L.body_syms) // 26
        nb = 9 * words; stride = nb + (nb & 1)
        clean = torch.zeros(N * stride + 64, dtype=torch.uint8, device="cuda")
        one = torch.zeros(nb + 64, dtype=torch.uint8, device="cuda")
        for f in range(N):
            d_px = torch.from_numpy(ol.oracle().lcg_pixels(n_px, 12345 + f).view(np.uint8)).cuda()
            t3.encode_frame_dev(d_px.data_ptr(), n_px, cfg, one.data_ptr(), words, s)
            clean[f * stride: f * stride + nb].copy_(one[:nb])
        torch.cuda.synchronize()
        work = torch.zeros_like(clean)
        ver = torch.zeros(nw * N, dtype=torch.int32, device="cuda")
        W, V = work.data_ptr(), ver.data_ptr()
        if side == "A":
            def op():
                for f in range(N):
                    t3.repair_erasures_frame_async(W + f * stride, words, cfg, n_raw, t3.REPAIR_WRITE, V + 24 * f, s)
        elif side == "B":
            def op(): t3.repair_erasures_frames_async(W, words, stride, N, cfg, n_raw, t3.REPAIR_WRITE, V, s)
        else:
            def op(): t3.repair_frames_async(W, words, stride, N, cfg, n_raw, t3.REPAIR_WRITE, V, s)
        for wl in ("clean", "err", "bytes")[: 2 if side == "C" else 3]:
            pristine = clean.clone()
            if wl == "err":
                for f in range(N):
                    one[:nb].copy_(pristine[f * stride: f * stride + nb])
                    t3.inject_errors_dev(one.data_ptr(), L.header_syms, nblk, 4242 + f, 3, s)
                    pristine[f * stride: f * stride + nb].copy_(one[:nb])
            if wl == "bytes":
                host = clean.cpu().numpy().copy()
                for f in range(N):
                    corrupt_bytes(host[f * stride + hs: f * stride + hs + 26 * nblk].reshape(nblk, 26), SEED + f)
                pristine = torch.from_numpy(host).cuda()
            torch.cuda.synchronize()
            res = {"side": side, "batch": label, "frames": N, "workload": wl, "lib": "T3HIP_LIB (another build)" if os.environ.get("T3HIP_LIB") else "this tree",
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
            res["verdict_sum"] = [int(x) for x in ver.cpu().numpy().reshape(N, nw).sum(axis=0)]
            res["batch_sha"] = hashlib.sha256(work.cpu().numpy().tobytes()).hexdigest()[:16]
            body = lambda t: torch.stack([t[f * stride + hs: f * stride + hs + 26 * nblk] for f in range(N)]).view(N * nblk, 26)
            damaged = (body(pristine) != body(clean)).any(dim=1)
            back = (body(work) == body(clean)).all(dim=1)
            res["blocks"], res["damaged"], res["recovered"] = N * nblk, int(damaged.sum()), int((damaged & back).sum())
            print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", choices=("A", "B", "C"))
    ap.add_argument("--warm", type=int, default=100); ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if a.side:
        return one_side(a.side, a.warm, a.reps)
    lib_a = os.environ.get("T3HIP_LIB_A")
    for side in ["A", "B", "C"] * a.rounds:
        env = dict(os.environ)
        env.pop("T3HIP_LIB", None)
        if side in ("A", "C") and lib_a: env["T3HIP_LIB"] = lib_a
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--side", side, "--warm", str(a.warm), "--reps", str(a.reps)],
                           env=env, capture_output=True, text=True, timeout=280)
        if r.returncode != 0:                                        # a side that failed ends the measurement: nothing more is started on the device
            sys.exit("erasures_frames_time: side %s failed (%d)\n%s" % (side, r.returncode, (r.stdout + r.stderr)[-3000:]))
        print("\n".join(x for x in r.stdout.strip().splitlines() if x.startswith("{")), flush=True)


if __name__ == "__main__":
    main()
