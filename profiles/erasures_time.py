"""Repair with erasures against the plain repair on an 8K FIXED RS(26,20) frame (profiles/erasures/notes.md).
    python3 profiles/erasures_time.py                  the whole measurement: A B A B A B, every side in a process of its own
    python3 profiles/erasures_time.py --side A         one side: one JSON line per workload
A = t3hip_repair_frame_async on the build T3HIP_LIB_A names (the parent's libt3hip.so; this tree's when unset).
B = t3hip_repair_erasures_frame_async on this tree's build.  Both with T3_REPAIR_WRITE.  Three workloads:
  clean   a clean frame
  err     the bench workload's 0..3 trit errors per block (t3hip_inject_errors_dev): no byte above 26
  bytes   byte corruption: per block 0..6 bytes replaced by uniform random bytes, from a counter hash of (seed, block)
Every repetition works on a fresh copy of the frame: a device-to-device copy from a pristine buffer in front of the repetition's first
event.  Events without the system fence (t3hip_event_*), one pair per repetition, 100 warm and 200 timed repetitions; mean, minimum and
maximum per repetition in microseconds.  For `bytes` each side also reports the damaged blocks (received != clean) it returned clean,
and checks its outcome block by block on a seeded sample against the CPU: the oracle's errors-only decoder on the residues for A, the
yardstick of tests/erasure_patterns.py for B."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FW, FH = 7680, 4320
SEED, SAMPLE = 20261020, 1500


def mix(x):
    """splitmix64 finaliser on a uint64 array"""
    import numpy as np
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def corrupt_bytes(body, seed):
    """body (n_blocks, 26) uint8, in place: block i gets h % 7 bytes replaced, at distinct positions p0 + q step (step odd, not 13),
    by uniform random bytes, all from a counter hash of (seed, i)"""
    import numpy as np
    with np.errstate(over="ignore"):
        i = np.arange(len(body), dtype=np.uint64)
        h = mix(i * np.uint64(0x9E3779B97F4A7C15) + np.uint64(seed))
        cnt = (h % np.uint64(7)).astype(np.int64)
        p0 = ((h >> np.uint64(8)) % np.uint64(26)).astype(np.int64); step = 1 + 2 * ((h >> np.uint64(16)) % np.uint64(6)).astype(np.int64)
        for q in range(6):
            rows = np.flatnonzero(cnt > q)
            v = (mix(h[rows] + np.uint64(q + 1)) >> np.uint64(24)) & np.uint64(0xFF)
            body[rows, (p0[rows] + q * step[rows]) % 26] = v.astype(np.uint8)


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
    hs, nblk = int(L.header_syms), int(L.body_syms) // 26
    s = torch.cuda.current_stream().cuda_stream
    d_px = torch.from_numpy(ol.oracle().lcg_pixels(n_px, 12345).view(np.uint8)).cuda()
    clean = torch.zeros(9 * words + 64, dtype=torch.uint8, device="cuda")
    t3.encode_frame_dev(d_px.data_ptr(), n_px, cfg, clean.data_ptr(), words, s)
    torch.cuda.synchronize()
    work = torch.zeros_like(clean)
    ver = torch.zeros(8, dtype=torch.int32, device="cuda")
    W, V = work.data_ptr(), ver.data_ptr()
    if side == "A":
        def op(): t3.repair_frame_async(W, words, cfg, n_raw, t3.REPAIR_WRITE, V, s)
    else:
        def op(): t3.repair_erasures_frame_async(W, words, cfg, n_raw, t3.REPAIR_WRITE, V, s)
    for wl in ("clean", "err", "bytes"):
        pristine = clean.clone()
        if wl == "err":
            t3.inject_errors_dev(pristine.data_ptr(), L.header_syms, nblk, 4242, 3, s)
        host = None
        if wl == "bytes":
            host = clean.cpu().numpy().copy()
            corrupt_bytes(host[hs: hs + 26 * nblk].reshape(nblk, 26), SEED)
            pristine = torch.from_numpy(host).cuda()
        torch.cuda.synchronize()
        res = {"side": side, "workload": wl, "lib": "T3HIP_LIB (another build)" if os.environ.get("T3HIP_LIB") else "this tree", "warm": warm, "reps": reps}
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
        res["verdict"] = ver.cpu().tolist()[: 4 if side == "A" else 6]
        body = lambda t: t[hs: hs + 26 * nblk].view(nblk, 26)
        damaged = (body(pristine) != body(clean)).any(dim=1)
        back = (body(work) == body(clean)).all(dim=1)
        res["blocks"], res["damaged"], res["recovered"] = nblk, int(damaged.sum()), int((damaged & back).sum())
        res["recovered_share"] = round(res["recovered"] / max(res["damaged"], 1), 5)
        if wl == "bytes":                                          # a seeded sample of damaged blocks, decided on the CPU
            import erasure_patterns as ep
            import rs_patterns as rp
            orc = ol.oracle(); F = rp.field(orc)
            rows = np.flatnonzero(damaged.cpu().numpy())
            rows = np.sort(np.random.default_rng(SEED).choice(rows, min(SAMPLE, len(rows)), replace=False))
            rec = host[hs: hs + 26 * nblk].reshape(nblk, 26)[rows]
            cl = clean.cpu().numpy()[hs: hs + 26 * nblk].reshape(nblk, 26)[rows]
            e = F.sub[rec % 27, cl]
            cw, _, ok = orc.rs_decode_blocks(20, e, mode=1)          # the errors-only rule on the residues
            want = (ok == 1) & ~cw.any(axis=1)                        # accepted, and as the clean block (no other codeword)
            if side == "B":
                for j in np.flatnonzero((rec > 26).any(axis=1)):
                    okj, c = ep.yardstick(orc).decide(20, e[j], rec[j] > 26)
                    want[j] = okj and not c.any()
            got = back.cpu().numpy()[rows]
            res["sample"], res["sample_recovered_cpu"], res["sample_recovered_gpu"] = len(rows), int(want.sum()), int(got.sum())
            res["sample_agrees"] = bool(np.array_equal(want, got))
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
        if side == "B" and os.environ.get("T3HIP_LIB_B"): env["T3HIP_LIB"] = os.environ["T3HIP_LIB_B"]     # a variant build of this tree
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--side", side, "--warm", str(a.warm), "--reps", str(a.reps)],
                           env=env, capture_output=True, text=True, timeout=280)
        if r.returncode != 0:                                    # a side that failed ends the measurement: nothing more is started on the device
            sys.exit("erasures_time: side %s failed (%d)\n%s" % (side, r.returncode, (r.stdout + r.stderr)[-3000:]))
        print("\n".join(x for x in r.stdout.strip().splitlines() if x.startswith("{")), flush=True)


if __name__ == "__main__":
    main()
