"""Decode with erasures in one call against repair-then-decode on an 8K FIXED RS(26,20) frame, pixel output
(profiles/decode_erasures/notes.md).
    python3 profiles/decode_erasures_time.py                  the whole measurement: A B A B A B, every side in a process of its own
    python3 profiles/decode_erasures_time.py --side A         one side: one JSON line per workload
A = the two calls of the build T3HIP_LIB_A names (the parent's libt3hip.so; this tree's when unset): t3hip_repair_erasures_frame_async
    with T3_REPAIR_WRITE on a copy of the frame, refreshed by a device-to-device copy OUTSIDE the timed events, then
    t3hip_decode_frame_async on it.
B = t3hip_decode_erasures_frame_async of this tree on the frame itself (it is never written: no copy).
Three workloads, as profiles/erasures_time.py builds them:
  clean   a clean frame
  err     the bench workload's 0..3 trit errors per block (t3hip_inject_errors_dev): no byte above 26
  bytes   byte corruption: per block 0..6 bytes replaced by uniform random bytes
Events without the system fence (t3hip_event_*), one pair per repetition, 100 warm and 200 timed repetitions; mean, minimum and maximum
per repetition in microseconds.  Each side also reports a SHA-256 of its pixels with the tiles that hold a refused block zeroed (the
tiles: those with a block the erasure repair, run once more untimed, does not bring back to the clean block); the driver compares them."""
import argparse
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "profiles"))
FW, FH = 7680, 4320
SEED = 20261020


def one_side(side, warm, reps):
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch
    import __graft_entry__ as g
    import oracle_lib as ol
    from erasures_time import corrupt_bytes
    t3 = g.load_package(); t3.init(0)
    n_px = FW * FH; n_raw = n_px // 2
    cfg = t3.make_cfg(profile=t3.ProfileID.P3_RS26_20, uep=2, mode=t3.MODE_FIXED)
    words = t3.encoded_words(n_raw, cfg); L = t3.plan(n_raw, cfg)
    hs, nblk = int(L.header_syms), int(L.body_syms) // 26
    s = torch.cuda.current_stream().cuda_stream
    d_px = torch.from_numpy(ol.oracle().lcg_pixels(n_px, 12345).view(np.uint8)).cuda()
    clean = torch.zeros(9 * words + 64, dtype=torch.uint8, device="cuda")
    t3.encode_frame_dev(d_px.data_ptr(), n_px, cfg, clean.data_ptr(), words, s)
    torch.cuda.synchronize()
    work = torch.zeros_like(clean)
    out = torch.zeros(6 * n_px + 64, dtype=torch.uint8, device="cuda")
    ver = torch.zeros(8, dtype=torch.int32, device="cuda")
    W, O, V = work.data_ptr(), out.data_ptr(), ver.data_ptr()
    for wl in ("clean", "err", "bytes"):
        pristine = clean.clone()
        if wl == "err":
            t3.inject_errors_dev(pristine.data_ptr(), L.header_syms, nblk, 4242, 3, s)
        if wl == "bytes":
            host = clean.cpu().numpy().copy()
            corrupt_bytes(host[hs: hs + 26 * nblk].reshape(nblk, 26), SEED)
            pristine = torch.from_numpy(host).cuda()
        P = pristine.data_ptr(); ref = pristine.clone()
        if side == "A":
            def op():
                t3.repair_erasures_frame_async(W, words, cfg, n_raw, t3.REPAIR_WRITE, V, s)
                t3.decode_frame_async(W, words, cfg, n_raw, O, n_px, V + 24, True, s)
        else:
            def op(): t3.decode_erasures_frame_async(P, words, cfg, n_raw, O, n_px, t3.FMT_PIXELS, V, s)
        torch.cuda.synchronize()
        res = {"side": side, "workload": wl, "lib": "T3HIP_LIB (another build)" if os.environ.get("T3HIP_LIB") else "this tree", "warm": warm, "reps": reps}
        for _ in range(warm):
            work.copy_(pristine); op()
        torch.cuda.synchronize()
        ev = [(t3.Event(), t3.Event()) for _ in range(reps)]
        for e0, e1 in ev:
            work.copy_(pristine)                                   # outside the timed events (B does not need it; both sides pay it alike)
            e0.record(s); op(); e1.record(s)
        torch.cuda.synchronize()
        us = [1000.0 * e0.elapsed_ms(e1) for e0, e1 in ev]
        res["us_mean"], res["us_min"], res["us_max"] = round(sum(us) / len(us), 2), round(min(us), 2), round(max(us), 2)
        v = ver.cpu().tolist()
        res["verdict"] = [v[0], v[1], v[4], v[5], "decode", v[6], v[7]] if side == "A" else v[:4]
        res["input_unchanged"] = bool(torch.equal(pristine, ref))
        # the tiles without a refused block: the erasure repair once more, untimed (both builds have it)
        work.copy_(pristine)
        t3.repair_erasures_frame_async(W, words, cfg, n_raw, t3.REPAIR_WRITE, V, s)
        torch.cuda.synchronize()
        back = (work[hs: hs + 26 * nblk].view(nblk, 26) == clean[hs: hs + 26 * nblk].view(nblk, 26)).all(dim=1).cpu().numpy()
        n_tiles = -(-max(int(L.band_blocks[b]) for b in range(9)) // 52)
        bad = np.zeros(n_tiles, bool)
        for b in range(9):
            f0 = int(L.band_body_off[b]) // 26
            m = np.flatnonzero(~back[f0: f0 + int(L.band_blocks[b])])
            bad[m // 52] = True
        px = out[: 6 * n_px].cpu().numpy().reshape(n_px, 6).copy()
        for t in np.flatnonzero(bad):
            px[t * 108 * 20: (t + 1) * 108 * 20] = 0
        res["tiles"], res["tiles_without_refused_block"] = int(n_tiles), int((~bad).sum())
        res["pixels_sha256_outside_refused_tiles"] = hashlib.sha256(px.tobytes()).hexdigest()[:16]
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
    sha = {}
    for side in ["A", "B"] * a.rounds:
        env = dict(os.environ)
        env.pop("T3HIP_LIB", None)
        if side == "A" and lib_a: env["T3HIP_LIB"] = lib_a
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--side", side, "--warm", str(a.warm), "--reps", str(a.reps)],
                           env=env, capture_output=True, text=True, timeout=280)
        if r.returncode != 0:                                    # a side that failed ends the measurement: nothing more is started on the device
            sys.exit("decode_erasures_time: side %s failed (%d)\n%s" % (side, r.returncode, (r.stdout + r.stderr)[-3000:]))
        for x in r.stdout.strip().splitlines():
            if x.startswith("{"):
                print(x, flush=True)
                d = json.loads(x); sha.setdefault(d["workload"], set()).add(d["pixels_sha256_outside_refused_tiles"])
    print(json.dumps({"outputs_equal_outside_refused_tiles": {w: len(v) == 1 for w, v in sha.items()}}), flush=True)


if __name__ == "__main__":
    main()
