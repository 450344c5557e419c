"""The reference decoder's stages 2 and 3 as separate kernels (t3_decode_stages.hip) on an 8K decoder-consistent stream: RS(26,20) on
every band, 20,766,720 body words (798,720 blocks per band, 143,769,600 output symbols), clean and with <= 3 symbol errors in ~30 % of
the blocks.  HIP events, warm-up, 10 launches each: time and algorithmic TB/s (descramble: 9 n bytes read + written; stage decode:
9 n read + the symbols written).  One JSON line.
    python3 profiles/stage_time.py           timings
    python3 profiles/stage_time.py --trace   one launch of each, plus t3hip_decode_profile_dev (COMPAT: dec_gather_rs_kernel) on the
                                             same stream, for rocprofv3 --kernel-trace --stats"""
import json, os, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as g
import oracle_lib as ol
from test_decode_stages import stage_body, N8K

t3 = g.load_package(); t3.init(0)
orc = ol.oracle()
trace = "--trace" in sys.argv
s = torch.cuda.current_stream().cuda_stream
KS, n = [24, 22, 20, 18], N8K


def stream_of(body, cfg):
    """header words (RS(26,18) codewords of the header, which the COMPAT decoder takes when clean) + the body scrambled with its seed"""
    hp = orc.header_pack(cfg, 0, 0)
    A = orc.rs_encode_blocks(18, hp[:18], mode=1)[0]
    B = orc.rs_encode_blocks(18, np.concatenate([hp[18:], np.zeros(9, np.uint8)]), mode=1)[0]
    flat = orc.scramble(body.reshape(-1), cfg.seed_a, cfg.seed_b, cfg.seed_s0, 0)
    return np.concatenate([A, B, np.zeros(2, np.uint8), flat])


def timed(f, reps=10):
    for _ in range(3): f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps): f()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


cfg = t3.make_cfg(profile=t3.ProfileID.P3_RS26_20, uep=2)
rng = np.random.default_rng(5)
res = []
for corrupt in (0, 3):
    body = stage_body(orc, rng, cfg, KS, (1, 1, 1, 1), n, corrupt)
    d_stream = torch.from_numpy(stream_of(body, cfg)).cuda()
    d_body = torch.from_numpy(body.reshape(-1).copy()).cuda()                    # the descrambled body (stage 3's input)
    d_scr = d_stream[54:].clone()                                                 # the scrambled body (stage 2's input)
    total = t3.demap_rsdecode_bands_syms(n, cfg, KS)
    d_out = torch.empty(total, dtype=torch.uint8, device="cuda"); d_nv = torch.zeros(1, dtype=torch.int64, device="cuda")
    reps = 1 if trace else 10
    ms = timed(lambda: t3.descramble_words_dev(d_scr.data_ptr(), n, cfg.seed_a, cfg.seed_b, cfg.seed_s0, s), reps)
    res.append({"kernel": "descramble_words", "errors": corrupt, "ms": round(ms, 4), "TBps": round(18 * n / ms / 1e9, 3)})
    for mode in (0, 1):
        ms = timed(lambda: t3.demap_rsdecode_bands_dev(d_body.data_ptr(), n, cfg, KS, (mode,) * 4, d_out.data_ptr(), total, d_nv.data_ptr(), s), reps)
        torch.cuda.synchronize()
        res.append({"kernel": "stage_decode", "mode": mode, "errors": corrupt, "ms": round(ms, 4), "TBps": round((9 * n + total) / ms / 1e9, 3),
                    "n_valid": int(d_nv.item()), "total": total})
    if trace:                                                                     # dec_gather_rs_kernel on the same stream (COMPAT)
        nw = len(d_stream) // 9; d_raw = torch.empty((nw + 16) * 9, dtype=torch.uint8, device="cuda")
        seen = t3.make_cfg()
        rc, nout = t3.decode_profile_dev(d_stream.data_ptr(), nw, seen, d_raw.data_ptr(), nw + 16, False, s)
        torch.cuda.synchronize()
        res.append({"path": "decode_profile_dev COMPAT", "errors": corrupt, "rc": rc, "n_out": nout})
print(json.dumps({"stream_words": n + 6, "body_words": n, "results": res}))
