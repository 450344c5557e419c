"""The records of a batch of equal frames in one call against a loop of single-frame record calls, and the containers' payload CRC the
same way (profiles/frame_records/notes.md): the payload is the coded output of FIXED RS(26,20) frames.
    python3 profiles/frame_records_time.py                                     the whole measurement: for both pairs and every shape, A B A B A B in processes of their own
    python3 profiles/frame_records_time.py --what rec --side A --shape 0       one side, one shape: one JSON line
--what rec:  A = a loop of frame_record_dev calls, one per frame, each on its own 8,256 bytes of scratch, on the build T3HIP_LIB_A names (the
             parent's libt3hip.so; this tree's when unset).  B = one frame_records_dev call on this tree's build, on the same scratch.
--what crc:  A = a loop of crc32_dev calls (each synchronises), B = one crc32_frames_dev call (one synchronisation).
Both sides on the same buffers: one frame's pixels coded once, copied to the batch's minimum stride, a different error pattern injected into
every copy (so the frames differ).  Events (without the system fence, t3hip_event_*) around the whole sequence of one repetition, 100 warm
and 200 timed repetitions, the mean per repetition in microseconds; the crc pair's figure therefore contains its synchronisations, which is
what it is about.  --reps / --warm: other counts (a kernel-trace run wants few).  "crc_xor" / "sym_sum": over all frames, equal on both sides."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(16, 854, 480), (16, 960, 540), (8, 1920, 1080), (4, 7680, 4320)]           # (frames, width, height); the last is informative


def one_side(what, side, shape, warm, reps):
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch
    import __graft_entry__ as g
    import oracle_lib as ol
    t3 = g.load_package(); t3.init(0)
    n, fw, fh = SHAPES[shape]; n_px = fw * fh; n_raw = n_px // 2
    cfg = t3.make_cfg(profile=t3.ProfileID.P3_RS26_20, uep=2, mode=t3.MODE_FIXED)
    words = t3.encoded_words(n_raw, cfg); L = t3.plan(n_raw, cfg)
    stride = (9 * words + 15) & ~15
    s = torch.cuda.current_stream().cuda_stream
    d_px = torch.from_numpy(ol.oracle().lcg_pixels(n_px, 12345).view(np.uint8)).cuda()
    d_cod = torch.zeros(n * stride + 64, dtype=torch.uint8, device="cuda")
    C_ = d_cod.data_ptr()
    t3.encode_frame_dev(d_px.data_ptr(), n_px, cfg, C_, words, s)
    torch.cuda.synchronize()
    for f in range(1, n): d_cod[f * stride: f * stride + 9 * words] = d_cod[: 9 * words]
    for f in range(n): t3.inject_errors_dev(C_ + f * stride, L.header_syms, L.body_syms // 26, 4242 + f, 3, s)
    torch.cuda.synchronize()
    slot = t3.frame_record_scratch_bytes(words)
    d_scr = torch.zeros(n * slot, dtype=torch.uint8, device="cuda"); d_rec = torch.zeros((n, t3.FRAME_RECORD_BYTES), dtype=torch.uint8, device="cuda")
    S, R = d_scr.data_ptr(), d_rec.data_ptr()
    crcs = [0] * n
    if what == "rec" and side == "A":
        def run():
            for f in range(n): t3.frame_record_dev(C_ + f * stride, words, f, cfg, R + f * t3.FRAME_RECORD_BYTES, S + f * slot, slot, s)
    elif what == "rec":
        def run(): t3.frame_records_dev(C_, words, stride, n, 0, 1, cfg, R, S, n * slot, s)
    elif side == "A":
        def run():
            for f in range(n): crcs[f] = t3.crc32_dev(C_ + f * stride, 9 * words, s)
    else:
        def run(): crcs[:] = t3.crc32_frames_dev(C_, 9 * words, stride, n, s)
    res = {"what": what, "side": side, "shape": "%d x %dx%d" % (n, fw, fh), "words": words, "lib": os.path.basename(os.path.dirname(t3.LIB_PATH)), "warm": warm, "reps": reps}
    for _ in range(warm): run()
    torch.cuda.synchronize()
    e0, e1 = t3.Event(), t3.Event()
    e0.record(s)
    for _ in range(reps): run()
    e1.record(s)
    torch.cuda.synchronize()
    res["us"] = round(1000.0 * e0.elapsed_ms(e1) / reps, 2)
    if what == "rec":
        recs = t3.index_assemble(d_rec.cpu().numpy().reshape(-1), 0)
        assert [r.frame_idx for r in recs] == list(range(n))
        crcs = [r.crc32 for r in recs]; res["sym_sum"] = sum(r.sym_sum for r in recs)
    x = 0
    for c in crcs: x ^= c
    res["crc_xor"] = x; res["crc_distinct"] = len(set(crcs))
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=["rec", "crc"]); ap.add_argument("--side", choices=["A", "B"]); ap.add_argument("--shape", type=int, default=0)
    ap.add_argument("--warm", type=int, default=100); ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if a.side:
        return one_side(a.what or "rec", a.side, a.shape, a.warm, a.reps)
    lib_a = os.environ.get("T3HIP_LIB_A")
    for what in ([a.what] if a.what else ["rec", "crc"]):
        for shape in range(len(SHAPES)):
            for _ in range(a.rounds):
                for side in ("A", "B"):
                    env = dict(os.environ)
                    env.pop("T3HIP_LIB", None)
                    if side == "A" and lib_a: env["T3HIP_LIB"] = lib_a
                    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--what", what, "--side", side, "--shape", str(shape), "--warm", str(a.warm),
                                        "--reps", str(a.reps)], env=env, capture_output=True, text=True, timeout=280)
                    if r.returncode != 0:                        # a side that failed ends the measurement: nothing more is started on the device
                        sys.exit("frame_records_time: %s %s shape %d failed (%d)\n%s" % (what, side, shape, r.returncode, (r.stdout + r.stderr)[-3000:]))
                    print(r.stdout.strip().splitlines()[-1], flush=True)


if __name__ == "__main__":
    main()
