"""The same pixel window out of every frame of a batch, decoded with erasures in one launch, against what a caller had before
(profiles/decode_erasures_frames_window/notes.md).
    python3 profiles/decode_erasures_frames_window_time.py [--warm 50] [--reps 100]      one JSON line per (batch, workload, output format)
Contenders, alternating repetition by repetition in ONE process, an event pair around every call:
  a  a loop of t3hip_decode_erasures_window_async over the frames: one verdict memset, one optional zero-fill and one launch per frame
  b  t3hip_decode_frames_window_async on the same window (bytes reduced mod 27, no erasure stage; workloads clean and err only)
  c  t3hip_decode_erasures_frames_window_async
Batches (FIXED RS(26,20), centred windows): 16 frames of 854 x 480 with the 427 x 240 window, 8 frames of 1920 x 1080 with the 854 x 480
window, 4 frames of 7680 x 4320 with the S15 854 x 480 window; frames 16-byte strides apart (b asks for that).
Workloads, as profiles/decode_erasures_time.py builds them: clean; err = 0..3 trit errors per block, no byte above 26; bytes = per block
0..6 bytes replaced by uniform random bytes (most blocks flagged).  Events without the system fence (t3hip_event_*); mean, minimum and
maximum per repetition in microseconds.  Each line also says whether c's four words equal a's for every frame, whether c's windows equal
a's outside the pixel tiles that hold a refused block (the tiles: those with a block the batched erasure repair, run once untimed, does
not bring back to the clean block), and whether the input came back unchanged."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "profiles"))
SEED = 20261021
BATCHES = (("16 x 854x480, window 427x240", 854, 480, 16, 427, 240), ("8 x 1920x1080, window 854x480", 1920, 1080, 8, 854, 480),
           ("4 x 7680x4320, window S15 854x480", 7680, 4320, 4, 854, 480))


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
    cfg = t3.make_cfg(profile=t3.ProfileID.P3_RS26_20, uep=2, mode=t3.MODE_FIXED)
    s = torch.cuda.current_stream().cuda_stream
    for label, FW, FH, N, w, h in BATCHES:
        n_px = FW * FH; n_raw = n_px // 2
        words = t3.encoded_words(n_raw, cfg); L = t3.plan(n_raw, cfg)
        hs, nblk = int(L.header_syms), int(L.body_syms) // 26
        nb = 9 * words; stride = (nb + 15) & ~15
        n_tiles = -(-max(int(L.band_blocks[b]) for b in range(9)) // 52)
        x0, y0 = (FW - w) // 2, (FH - h) // 2
        clean = torch.zeros(N * stride + 64, dtype=torch.uint8, device="cuda")
        one = torch.zeros(nb + 64, dtype=torch.uint8, device="cuda")
        for f in range(N):
            d_px = torch.from_numpy(ol.oracle().lcg_pixels(n_px, 12345 + f).view(np.uint8)).cuda()
            t3.encode_frame_dev(d_px.data_ptr(), n_px, cfg, one.data_ptr(), words, s)
            clean[f * stride: f * stride + nb].copy_(one[:nb])
        torch.cuda.synchronize()
        work = torch.zeros_like(clean)
        ostride = (6 * w * h + 15) & ~15                                    # (the pixel format's; RGB8 uses the same stride)
        out_a = torch.zeros(N * ostride + 64, dtype=torch.uint8, device="cuda"); out_b = torch.zeros_like(out_a); out_c = torch.zeros_like(out_a)
        ver = torch.zeros(4 * N + 4 * N + 2 * N + 6 * N, dtype=torch.int32, device="cuda")
        OA, OB, OC, V = out_a.data_ptr(), out_b.data_ptr(), out_c.data_ptr(), ver.data_ptr()
        VA, VC, VB, VR = V, V + 16 * N, V + 32 * N, V + 40 * N
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
            # the tiles without a refused block, per frame: the batched erasure repair on a copy, untimed
            work.copy_(pristine)
            t3.repair_erasures_frames_async(work.data_ptr(), words, stride, N, cfg, n_raw, t3.REPAIR_WRITE, VR, s)
            torch.cuda.synchronize()
            good_px = []
            for f in range(N):
                lo = f * stride + hs
                back = (work[lo: lo + 26 * nblk].view(nblk, 26) == clean[lo: lo + 26 * nblk].view(nblk, 26)).all(dim=1).cpu().numpy()
                bad = np.zeros(n_tiles, bool)
                for b in range(9):
                    f0 = int(L.band_body_off[b]) // 26
                    bad[np.flatnonzero(~back[f0: f0 + int(L.band_blocks[b])]) // 52] = True
                good_px.append(np.repeat(~bad, 108 * 20)[:n_px].reshape(FH, FW)[y0: y0 + h, x0: x0 + w].copy())
            for fmt, fname in ((t3.FMT_PIXELS, "pixels"), (t3.FMT_RGB, "rgb8")):
                ub = 6 if fmt == t3.FMT_PIXELS else 3

                def loop():
                    for f in range(N):
                        t3.decode_erasures_window_async(P + f * stride, words, cfg, n_raw, FW, FH, x0, y0, w, h, OA + f * ostride, fmt, VA + 16 * f, s)
                ops = {"a": loop, "c": lambda: t3.decode_erasures_frames_window_async(P, words, stride, N, cfg, n_raw, FW, FH, x0, y0, w, h, OC, ostride, fmt, VC, s)}
                if wl != "bytes":
                    ops["b"] = lambda: t3.decode_frames_window_async(P, words, stride, N, cfg, n_raw, FW, FH, x0, y0, w, h, OB, ostride, fmt, VB, s)
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
                fp = t3.decode_erasures_frames_window_plan(n_raw, N, cfg, FW, FH, x0, y0, w, h, fmt)
                res = {"batch": label, "frames": N, "workload": wl, "out": fname, "one_launch": int(fp.one_launch), "tickets": int(fp.tiles_launched),
                       "tiles_per_frame": int(n_tiles), "zero_fill": int(fp.frame.zero_fill), "warm": a.warm, "reps": a.reps}
                for k in order:
                    us = [1000.0 * e0.elapsed_ms(e1) for e0, e1 in ev[k]]
                    res[k + "_us"] = [round(sum(us) / len(us), 2), round(min(us), 2), round(max(us), 2)]
                v = ver.cpu().numpy()
                va, vc = v[: 4 * N].reshape(N, 4), v[4 * N: 8 * N].reshape(N, 4)
                res["c_words_equal_a_per_frame"] = bool(np.array_equal(va, vc))
                res["words_sum"] = [int(x) for x in vc.sum(axis=0)]
                same = True; compared = 0.0
                for f in range(N):
                    wa = out_a[f * ostride: f * ostride + ub * w * h].cpu().numpy().reshape(h, w, ub)
                    wc = out_c[f * ostride: f * ostride + ub * w * h].cpu().numpy().reshape(h, w, ub)
                    same &= bool(np.array_equal(wa[good_px[f]], wc[good_px[f]])); compared += float(good_px[f].mean()) / N
                res["c_bytes_equal_a_outside_refused_tiles"] = same
                res["window_px_compared"] = round(compared, 4)
                res["input_unchanged"] = bool(torch.equal(pristine, ref))
                print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
