"""A pixel window decoded with erasures in one launch against what a caller had before, on an 8K FIXED RS(26,20) frame
(profiles/decode_erasures_window/notes.md).
    python3 profiles/decode_erasures_window_time.py [--warm 50] [--reps 100]      one JSON line per (output format, workload, window)
Contenders, alternating repetition by repetition in ONE process, an event pair around every call:
  a  t3hip_decode_erasures_frame_async on the whole frame, no crop counted: a lower bound for what a caller of the parent pays
  b  t3hip_decode_window_async on the same window (bytes reduced mod 27, no erasure stage; workloads clean and err only)
  c  t3hip_decode_erasures_window_async
Windows (centred on the 7680 x 4320 frame): S15 854 x 480 (0.111 of the tiles), 1920 x 1080, and the full frame.
Workloads, as profiles/decode_erasures_time.py builds them: clean; err = 0..3 trit errors per block, no byte above 26; bytes = per block
0..6 bytes replaced by uniform random bytes (most blocks flagged).  Events without the system fence (t3hip_event_*); mean, minimum and
maximum per repetition in microseconds.  Each line also says whether c's window equals the numpy crop of a's output outside the pixel
tiles that hold a refused block (the tiles: those with a block the erasure repair, run once untimed, does not bring back to the clean
block), and whether the input came back unchanged."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "profiles"))
FW, FH = 7680, 4320
SEED = 20261020
WINDOWS = (("S15 854x480", 854, 480), ("1920x1080", 1920, 1080), ("full frame", FW, FH))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warm", type=int, default=50); ap.add_argument("--reps", type=int, default=100)
    a = ap.parse_args()
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
    full = torch.zeros(6 * n_px + 64, dtype=torch.uint8, device="cuda")
    wout = torch.zeros(6 * n_px + 64, dtype=torch.uint8, device="cuda")
    ver = torch.zeros(16, dtype=torch.int32, device="cuda")
    O, WO, V = full.data_ptr(), wout.data_ptr(), ver.data_ptr()
    n_tiles = -(-max(int(L.band_blocks[b]) for b in range(9)) // 52)
    for wl in ("clean", "err", "bytes"):
        pristine = clean.clone()
        if wl == "err":
            t3.inject_errors_dev(pristine.data_ptr(), L.header_syms, nblk, 4242, 3, s)
        if wl == "bytes":
            host = clean.cpu().numpy().copy()
            corrupt_bytes(host[hs: hs + 26 * nblk].reshape(nblk, 26), SEED)
            pristine = torch.from_numpy(host).cuda()
        P = pristine.data_ptr(); ref = pristine.clone()
        # the tiles without a refused block: the erasure repair on a copy, untimed
        work.copy_(pristine)
        t3.repair_erasures_frame_async(work.data_ptr(), words, cfg, n_raw, t3.REPAIR_WRITE, V + 32, s)
        torch.cuda.synchronize()
        back = (work[hs: hs + 26 * nblk].view(nblk, 26) == clean[hs: hs + 26 * nblk].view(nblk, 26)).all(dim=1).cpu().numpy()
        bad = np.zeros(n_tiles, bool)
        for b in range(9):
            f0 = int(L.band_body_off[b]) // 26
            bad[np.flatnonzero(~back[f0: f0 + int(L.band_blocks[b])]) // 52] = True
        good_px = np.repeat(~bad, 108 * 20)[:n_px].reshape(FH, FW)
        for fmt, fname in ((t3.FMT_PIXELS, "pixels"), (t3.FMT_RGB, "rgb8")):
            ub = 6 if fmt == t3.FMT_PIXELS else 3
            for label, w, h in WINDOWS:
                x0, y0 = (FW - w) // 2, (FH - h) // 2
                ops = {"a": lambda: t3.decode_erasures_frame_async(P, words, cfg, n_raw, O, n_px, fmt, V, s),
                       "c": lambda: t3.decode_erasures_window_async(P, words, cfg, n_raw, FW, FH, x0, y0, w, h, WO, fmt, V + 16, s)}
                if wl != "bytes":
                    ops["b"] = lambda: t3.decode_window_async(P, words, cfg, n_raw, FW, FH, x0, y0, w, h, WO, fmt, V + 32, s)
                order = sorted(ops)
                for _ in range(a.warm):
                    for k in order: ops[k]()
                torch.cuda.synchronize()
                ev = {k: [(t3.Event(), t3.Event()) for _ in range(a.reps)] for k in order}
                for i in range(a.reps):
                    for k in order[i % len(order):] + order[: i % len(order)]:           # the contenders in turn, the first one rotating
                        e0, e1 = ev[k][i]
                        e0.record(s); ops[k](); e1.record(s)
                torch.cuda.synchronize()
                wp = t3.decode_erasures_window_plan(n_raw, cfg, FW, FH, x0, y0, w, h, fmt)
                res = {"workload": wl, "out": fname, "window": label, "tiles_launched": int(wp.tiles_launched), "tiles": int(n_tiles), "zero_fill": int(wp.zero_fill),
                       "warm": a.warm, "reps": a.reps}
                for k in order:
                    us = [1000.0 * e0.elapsed_ms(e1) for e0, e1 in ev[k]]
                    res[k + "_us"] = [round(sum(us) / len(us), 2), round(min(us), 2), round(max(us), 2)]
                ops["a"](); ops["c"]()                                                      # c last: wout holds its window
                torch.cuda.synchronize()
                v = ver.cpu().tolist()
                res["a_words"], res["c_words"] = v[0:4], v[4:8]
                fa = full[: ub * n_px].cpu().numpy().reshape(FH, FW, ub)[y0: y0 + h, x0: x0 + w]
                wc = wout[: ub * w * h].cpu().numpy().reshape(h, w, ub)
                keep = good_px[y0: y0 + h, x0: x0 + w]
                res["window_equals_crop_outside_refused_tiles"] = bool(np.array_equal(fa[keep], wc[keep]))
                res["window_px_compared"] = float(round(keep.mean(), 4))
                res["input_unchanged"] = bool(torch.equal(pristine, ref))
                print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
