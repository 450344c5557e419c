"""Decode with erasures of a batch of equal FIXED RS(26,20) frames, pixel output, the input read-only: ONE
t3hip_decode_erasures_frames_async call against a loop of t3hip_decode_erasures_frame_async over the frames, and against the batched
repair with erasures followed by the batched decode (profiles/decode_erasures_frames/notes.md).
    python3 profiles/decode_erasures_frames_time.py             the whole measurement: A B C A B C A B C (A and B alternate), every side in
                                                                a process of its own
    python3 profiles/decode_erasures_frames_time.py --side A    one side: one JSON line per batch and workload
A = a loop of N t3hip_decode_erasures_frame_async calls, on the build T3HIP_LIB_A names (the parent's libt3hip.so; this tree's when unset).
B = one t3hip_decode_erasures_frames_async call on this tree's build.
C = the build T3HIP_LIB_A names: t3hip_repair_erasures_frames_async with T3_REPAIR_WRITE on a copy of the batch, refreshed by a
    device-to-device copy OUTSIDE the timed events, then t3hip_decode_frames_async on it -- the only other route to a batch; it needs a
    writable buffer and moves the coded bytes twice.
Batches: 16 frames of 854 x 480 and 8 frames of 1920 x 1080; frame f at f * stride, stride = the frame's bytes rounded up to 16 (the
plain batch decoder of side C asks for it; A and B take any even stride), its pixels at f * out_stride, out_stride = 6 * pixels rounded up
to 16.  The three workloads of profiles/erasures/notes.md section 2:
  clean   clean frames
  err     the bench workload's 0..3 trit errors per block (t3hip_inject_errors_dev, a seed per frame): no byte above 26
  bytes   byte corruption: per block 0..6 bytes replaced by uniform random bytes (erasures_time.corrupt_bytes, a seed per frame)
Events without the system fence (t3hip_event_*), one pair per repetition, 100 warm and 200 timed repetitions; mean, minimum and maximum
per repetition in microseconds.  Each line also holds input_unchanged (the coded batch after the last repetition against a copy taken
before the first), the per-word sums of the frames' four words, and a SHA-256 of the pixels with the tiles that hold a refused block
zeroed (the tiles: those with a block the batched erasure repair, run once more untimed, does not bring back to the clean block); the
driver compares sums and hashes between the sides."""
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
    for label, fw, fh, N in BATCHES:
        n_px = fw * fh; n_raw = n_px // 2
        words = t3.encoded_words(n_raw, cfg); L = t3.plan(n_raw, cfg)
        hs, nblk = int(L.header_syms), int(L.body_syms) // 26
        nb = 9 * words; stride = (nb + 15) & ~15; ob = 6 * n_px; ostride = (ob + 15) & ~15
        clean = torch.zeros(N * stride + 64, dtype=torch.uint8, device="cuda")
        one = torch.zeros(nb + 64, dtype=torch.uint8, device="cuda")
        for f in range(N):
            d_px = torch.from_numpy(ol.oracle().lcg_pixels(n_px, 12345 + f).view(np.uint8)).cuda()
            t3.encode_frame_dev(d_px.data_ptr(), n_px, cfg, one.data_ptr(), words, s)
            clean[f * stride: f * stride + nb].copy_(one[:nb])
        torch.cuda.synchronize()
        work = torch.zeros_like(clean)
        out = torch.zeros(N * ostride + 64, dtype=torch.uint8, device="cuda")
        ver = torch.zeros(6 * N + 2 * N, dtype=torch.int32, device="cuda")
        W, O, V = work.data_ptr(), out.data_ptr(), ver.data_ptr()
        for wl in ("clean", "err", "bytes"):
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
            P = pristine.data_ptr(); ref = pristine.clone()
            if side == "A":
                def op():
                    for f in range(N):
                        t3.decode_erasures_frame_async(P + f * stride, words, cfg, n_raw, O + f * ostride, n_px, t3.FMT_PIXELS, V + 16 * f, s)
            elif side == "B":
                def op(): t3.decode_erasures_frames_async(P, words, stride, N, cfg, n_raw, O, ostride, t3.FMT_PIXELS, V, s)
            else:
                def op():
                    t3.repair_erasures_frames_async(W, words, stride, N, cfg, n_raw, t3.REPAIR_WRITE, V, s)
                    t3.decode_frames_async(W, words, stride, N, cfg, n_raw, O, ostride, t3.FMT_PIXELS, V + 24 * N, s)
            res = {"side": side, "batch": label, "frames": N, "workload": wl, "lib": "T3HIP_LIB (another build)" if os.environ.get("T3HIP_LIB") else "this tree",
                   "warm": warm, "reps": reps}
            for _ in range(warm):
                work.copy_(pristine); op()
            torch.cuda.synchronize()
            ev = [(t3.Event(), t3.Event()) for _ in range(reps)]
            for e0, e1 in ev:
                work.copy_(pristine)                               # outside the timed events (only C needs it; all sides pay it alike)
                e0.record(s); op(); e1.record(s)
            torch.cuda.synchronize()
            us = [1000.0 * e0.elapsed_ms(e1) for e0, e1 in ev]
            res["us_mean"], res["us_min"], res["us_max"] = round(sum(us) / len(us), 2), round(min(us), 2), round(max(us), 2)
            v = ver.cpu().numpy()
            if side == "C":                                        # the repair's words 0, 1, 4, 5: the four words of the erasure decoders
                res["verdict_sum"] = [int(x) for x in v[: 6 * N].reshape(N, 6)[:, [0, 1, 4, 5]].sum(axis=0)]
            else:
                res["verdict_sum"] = [int(x) for x in v[: 4 * N].reshape(N, 4).sum(axis=0)]
            res["input_unchanged"] = bool(torch.equal(pristine, ref))
            # the tiles without a refused block: the batched erasure repair once more, untimed (both builds have it)
            work.copy_(pristine)
            t3.repair_erasures_frames_async(W, words, stride, N, cfg, n_raw, t3.REPAIR_WRITE, V, s)
            torch.cuda.synchronize()
            n_tiles = -(-max(int(L.band_blocks[b]) for b in range(9)) // 52)
            h = hashlib.sha256(); good = 0
            for f in range(N):
                lo = f * stride + hs
                back = (work[lo: lo + 26 * nblk].view(nblk, 26) == clean[lo: lo + 26 * nblk].view(nblk, 26)).all(dim=1).cpu().numpy()
                bad = np.zeros(n_tiles, bool)
                for b in range(9):
                    f0 = int(L.band_body_off[b]) // 26
                    m = np.flatnonzero(~back[f0: f0 + int(L.band_blocks[b])])
                    bad[m // 52] = True
                px = out[f * ostride: f * ostride + ob].cpu().numpy().reshape(n_px, 6).copy()
                for t in np.flatnonzero(bad):
                    px[t * 108 * 20: (t + 1) * 108 * 20] = 0
                h.update(px.tobytes()); good += int((~bad).sum())
            res["tiles"], res["tiles_without_refused_block"] = int(N * n_tiles), good
            res["pixels_sha256_outside_refused_tiles"] = h.hexdigest()[:16]
            print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", choices=("A", "B", "C"))
    ap.add_argument("--sides", default="ABC")
    ap.add_argument("--warm", type=int, default=100); ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if a.side:
        return one_side(a.side, a.warm, a.reps)
    lib_a = os.environ.get("T3HIP_LIB_A")
    sha, sums = {}, {}
    for side in list(a.sides) * a.rounds:
        env = dict(os.environ)
        env.pop("T3HIP_LIB", None)
        if side in ("A", "C") and lib_a: env["T3HIP_LIB"] = lib_a
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--side", side, "--warm", str(a.warm), "--reps", str(a.reps)],
                           env=env, capture_output=True, text=True, timeout=400)
        if r.returncode != 0:                                        # a side that failed ends the measurement: nothing more is started on the device
            sys.exit("decode_erasures_frames_time: side %s failed (%d)\n%s" % (side, r.returncode, (r.stdout + r.stderr)[-3000:]))
        for x in r.stdout.strip().splitlines():
            if x.startswith("{"):
                print(x, flush=True)
                d = json.loads(x); key = d["batch"] + " " + d["workload"]
                sha.setdefault(key, set()).add(d["pixels_sha256_outside_refused_tiles"])
                if side != "C": sums.setdefault(key, set()).add(tuple(d["verdict_sum"]))
    print(json.dumps({"outputs_equal_outside_refused_tiles": {w: len(v) == 1 for w, v in sha.items()},
                      "verdict_sums_equal_A_B": {w: len(v) == 1 for w, v in sums.items()}}), flush=True)


if __name__ == "__main__":
    main()
