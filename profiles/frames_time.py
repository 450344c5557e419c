"""A batch of equal frames in one call against a loop of single-frame calls (profiles/frames/notes.md): FIXED RS(26,20), pixels, 0..3
symbol errors per block.
    python3 profiles/frames_time.py                       the whole measurement: for every shape, A B A B A B in processes of their own
    python3 profiles/frames_time.py --side A --shape 0    one side, one shape: one JSON line
A = a loop of encode_frame_dev / decode_frame_async calls, one per frame, on the build T3HIP_LIB_A names (the parent's libt3hip.so; this
tree's when unset).  B = one encode_frames_dev / decode_frames_async call on this tree's build.  Both on the same buffers: frames at the
batch's minimum strides.  Events (without the system fence, t3hip_event_*) around the whole sequence of one repetition, 100 warm and 200
timed repetitions, the mean per repetition in microseconds.  --reps / --warm: other counts (a kernel-trace run wants few)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(16, 854, 480), (8, 1920, 1080), (4, 3840, 2160)]


def one_side(side, shape, warm, reps):
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch
    import __graft_entry__ as g
    import oracle_lib as ol
    t3 = g.load_package(); t3.init(0)
    n, w, h = SHAPES[shape]; n_px = w * h; n_raw = n_px // 2
    cfg = t3.make_cfg(profile=t3.ProfileID.P3_RS26_20, uep=2, mode=t3.MODE_FIXED)
    words = t3.encoded_words(n_raw, cfg); L = t3.plan(n_raw, cfg)
    r16 = lambda x: (x + 15) & ~15
    s_px, s_cod = r16(6 * n_px), r16(9 * words)
    s = torch.cuda.current_stream().cuda_stream
    d_px = torch.zeros(n * s_px + 64, dtype=torch.uint8, device="cuda")
    for f in range(n):
        d_px[f * s_px: f * s_px + 6 * n_px] = torch.from_numpy(ol.oracle().lcg_pixels(n_px, 12345 + f).view(np.uint8)).cuda()
    d_cod = torch.zeros(n * s_cod + 64, dtype=torch.uint8, device="cuda")
    d_bad = torch.zeros(n * s_cod + 64, dtype=torch.uint8, device="cuda")
    d_out = torch.zeros(n * s_px + 64, dtype=torch.uint8, device="cuda")
    ver = torch.zeros(2 * n, dtype=torch.int32, device="cuda")
    P, C_, B_, O, V = d_px.data_ptr(), d_cod.data_ptr(), d_bad.data_ptr(), d_out.data_ptr(), ver.data_ptr()
    if side == "A":
        def enc():
            for f in range(n): t3.encode_frame_dev(P + f * s_px, n_px, cfg, C_ + f * s_cod, words, s)
        def dec():
            for f in range(n): t3.decode_frame_async(B_ + f * s_cod, words, cfg, n_raw, O + f * s_px, n_px, V + 8 * f, True, s)
    else:
        def enc(): t3.encode_frames_dev(P, n_px, t3.FRAMES_PIXELS, s_px, n, cfg, C_, s_cod, s)
        def dec(): t3.decode_frames_async(B_, words, s_cod, n, cfg, n_raw, O, s_px, t3.FRAMES_PIXELS, V, s)
    enc(); torch.cuda.synchronize()
    d_bad.copy_(d_cod)
    for f in range(n): t3.inject_errors_dev(B_ + f * s_cod, L.header_syms, L.body_syms // 26, 4242 + f, 3, s)
    res = {"side": side, "shape": "%d x %dx%d" % (n, w, h), "lib": os.path.basename(os.path.dirname(t3.LIB_PATH)), "warm": warm, "reps": reps}
    for name, fn in (("encode", enc), ("decode", dec)):
        for _ in range(warm): fn()
        torch.cuda.synchronize()
        e0, e1 = t3.Event(), t3.Event()
        e0.record(s)
        for _ in range(reps): fn()
        e1.record(s)
        res[name + "_us"] = round(1000.0 * e0.elapsed_ms(e1) / reps, 2)
    torch.cuda.synchronize()
    res["exact"] = bool(torch.equal(d_out[: n * s_px], d_px[: n * s_px])); res["verdict_sum"] = int(ver.abs().sum().item())
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
                    sys.exit("frames_time: %s shape %d failed (%d)\n%s" % (side, shape, r.returncode, (r.stdout + r.stderr)[-3000:]))
                print(r.stdout.strip().splitlines()[-1], flush=True)


if __name__ == "__main__":
    main()
