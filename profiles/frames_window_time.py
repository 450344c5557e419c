"""The same window out of a batch of equal frames in one call against a loop of single-frame window calls (profiles/frames_window/notes.md):
FIXED RS(26,20), RGB out, 0..3 symbol errors per block.
    python3 profiles/frames_window_time.py                       the whole measurement: for every shape, A B A B A B in processes of their own
    python3 profiles/frames_window_time.py --side A --shape 0    one side, one shape: one JSON line
A = a loop of decode_window_async calls, one per frame, on the build T3HIP_LIB_A names (the parent's libt3hip.so; this tree's when unset).
B = one decode_frames_window_async call on this tree's build.  Both on the same buffers: coded frames at the batch's minimum stride (one
frame's pixels coded once, a different error pattern injected into every copy), windows at the minimum output stride.  Events (without the
system fence, t3hip_event_*) around the whole sequence of one repetition, 100 warm and 200 timed repetitions, the mean per repetition in
microseconds.  --reps / --warm: other counts (a kernel-trace run wants few).  "sum" is the byte sum of all windows: equal on both sides."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (frames, fw, fh, window x0, y0, w, h): the S15 centre window of 8K frames, a 320 x 180 window of 960 x 540 frames, the S24 centre window of 8K frames
SHAPES = [(16, 7680, 4320, 3413, 1920, 854, 480), (16, 960, 540, 320, 180, 320, 180), (4, 7680, 4320, 1920, 1080, 3840, 2160)]


def one_side(side, shape, warm, reps):
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch
    import __graft_entry__ as g
    import oracle_lib as ol
    t3 = g.load_package(); t3.init(0)
    n, fw, fh, x0, y0, w, h = SHAPES[shape]; n_px = fw * fh; n_raw = n_px // 2
    cfg = t3.make_cfg(profile=t3.ProfileID.P3_RS26_20, uep=2, mode=t3.MODE_FIXED)
    words = t3.encoded_words(n_raw, cfg); L = t3.plan(n_raw, cfg)
    r16 = lambda x: (x + 15) & ~15
    s_cod, s_out = r16(9 * words), r16(3 * w * h)
    s = torch.cuda.current_stream().cuda_stream
    d_px = torch.from_numpy(ol.oracle().lcg_pixels(n_px, 12345).view(np.uint8)).cuda()
    d_cod = torch.zeros(n * s_cod + 64, dtype=torch.uint8, device="cuda")
    d_out = torch.zeros(n * s_out + 64, dtype=torch.uint8, device="cuda")
    ver = torch.zeros(2 * n, dtype=torch.int32, device="cuda")
    C_, O, V = d_cod.data_ptr(), d_out.data_ptr(), ver.data_ptr()
    t3.encode_frame_dev(d_px.data_ptr(), n_px, cfg, C_, words, s)
    torch.cuda.synchronize()
    for f in range(1, n): d_cod[f * s_cod: f * s_cod + 9 * words] = d_cod[: 9 * words]
    for f in range(n): t3.inject_errors_dev(C_ + f * s_cod, L.header_syms, L.body_syms // 26, 4242 + f, 3, s)
    torch.cuda.synchronize()
    if side == "A":
        def dec():
            for f in range(n): t3.decode_window_async(C_ + f * s_cod, words, cfg, n_raw, fw, fh, x0, y0, w, h, O + f * s_out, t3.WINDOW_RGB, V + 8 * f, s)
    else:
        def dec(): t3.decode_frames_window_async(C_, words, s_cod, n, cfg, n_raw, fw, fh, x0, y0, w, h, O, s_out, t3.WINDOW_RGB, V, s)
    res = {"side": side, "shape": "%d x (%dx%d of %dx%d)" % (n, w, h, fw, fh), "lib": os.path.basename(os.path.dirname(t3.LIB_PATH)), "warm": warm, "reps": reps}
    for _ in range(warm): dec()
    torch.cuda.synchronize()
    e0, e1 = t3.Event(), t3.Event()
    e0.record(s)
    for _ in range(reps): dec()
    e1.record(s)
    res["decode_us"] = round(1000.0 * e0.elapsed_ms(e1) / reps, 2)
    torch.cuda.synchronize()
    res["sum"] = int(d_out.sum(dtype=torch.int64).item()); res["verdict_sum"] = int(ver.abs().sum().item())
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", choices=["A", "B"]); ap.add_argument("--shape", type=int, default=0)
    ap.add_argument("--warm", type=int, default=100); ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if a.side:
        return one_side(a.side, a.shape, a.warm, a.reps)
    lib_a = os.environ.get("T3HIP_LIB_A")
    for shape in range(len(SHAPES)):
        for _ in range(a.rounds):
            for side in ("A", "B"):
                env = dict(os.environ)
                env.pop("T3HIP_LIB", None)
                if side == "A" and lib_a: env["T3HIP_LIB"] = lib_a
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--side", side, "--shape", str(shape), "--warm", str(a.warm), "--reps", str(a.reps)],
                                   env=env, capture_output=True, text=True, timeout=280)
                if r.returncode != 0:                            # a side that failed ends the measurement: nothing more is started on the device
                    sys.exit("frames_window_time: %s shape %d failed (%d)\n%s" % (side, shape, r.returncode, (r.stdout + r.stderr)[-3000:]))
                print(r.stdout.strip().splitlines()[-1], flush=True)


if __name__ == "__main__":
    main()
