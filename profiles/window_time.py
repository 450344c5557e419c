"""Window decode and image compose timing on one 8K C2 FIXED frame (P3, RS(26,20), 0..3 symbol errors per block: the bench's workload).

  baseline leg  what the library could do before the window decode existed, entry points of that version only, so that this leg runs
                unchanged on that version's build (T3HIP_LIB=<its libt3hip.so>): t3hip_decode_frame_async (pixels) ->
                t3hip_extract_center_q_dev -> t3hip_quant_to_rgb_dev per centred window; t3hip_blit_center_rgb_dev per target size
  new leg       t3hip_decode_window_async, RGB out, the same four centred windows; t3hip_image_compose_dev of a target-sized source, centred

argv: [baseline|new|both] [launches per sample] [samples] [out.json].  Each figure is the median over `samples` of the mean over
`launches` back-to-back calls (HIP events), after 200 warm-up calls of the full decode (80 ms of settling); the legs alternate
sample by sample.  One JSON object per run, appended to out.json as a line."""
import json, os, sys, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as g
import oracle_lib as ol
import numpy as np
leg = sys.argv[1] if len(sys.argv) > 1 else "both"
n = int(sys.argv[2]) if len(sys.argv) > 2 else 20
samples = int(sys.argv[3]) if len(sys.argv) > 3 else 9
out_path = sys.argv[4] if len(sys.argv) > 4 else None
t3 = g.load_package(); t3.init(0)
FW, FH = 7680, 4320; NPX = FW * FH
STD = {24: (3840, 2160), 21: (1920, 1080), 18: (1280, 720), 15: (854, 480)}
orc = ol.oracle()
d_px = torch.from_numpy(orc.lcg_pixels(NPX, 12345).view(np.uint8)).cuda()
s = torch.cuda.current_stream().cuda_stream
cfg = t3.make_cfg(profile=t3.ProfileID.P3_RS26_20, uep=2, mode=t3.MODE_FIXED)
n_raw = NPX // 2; n_enc = t3.encoded_words(n_raw, cfg)
coded = torch.zeros(n_enc * 9 + 64, dtype=torch.uint8, device="cuda")
t3.encode_frame_dev(d_px.data_ptr(), NPX, cfg, coded.data_ptr(), n_enc, s)
L = t3.plan(n_raw, cfg)
t3.inject_errors_dev(coded.data_ptr(), L.header_syms, L.body_syms // 26, 4242, 3, s)
full = torch.zeros(NPX * 6 + 64, dtype=torch.uint8, device="cuda")
sub_px = torch.zeros(3840 * 2160 * 6 + 64, dtype=torch.uint8, device="cuda")
rgb_a = torch.zeros(3840 * 2160 * 3 + 64, dtype=torch.uint8, device="cuda"); rgb_b = torch.zeros_like(rgb_a)
ver = torch.zeros(2, dtype=torch.int32, device="cuda")
canvas = torch.zeros(NPX * 3 + 64, dtype=torch.uint8, device="cuda")
src = torch.from_numpy(orc.lcg_rgb(3840 * 2160, 99)).cuda()


def base_window(sub):
    w, h = STD[sub]
    t3.decode_frame_async(coded.data_ptr(), n_enc, cfg, n_raw, full.data_ptr(), NPX, ver.data_ptr(), True, s)
    t3.extract_center_q_dev(full.data_ptr(), FW, FH, sub_px.data_ptr(), w, h, s)
    t3.quant_to_rgb_dev(sub_px.data_ptr(), w * h, rgb_a.data_ptr(), s)


def new_window(sub):
    w, h = STD[sub]
    t3.decode_window_async(coded.data_ptr(), n_enc, cfg, n_raw, FW, FH, (FW - w) // 2, (FH - h) // 2, w, h, rgb_b.data_ptr(), t3.WINDOW_RGB, ver.data_ptr(), s)


calls = {}
if leg in ("baseline", "both"):
    calls["base_full_decode"] = lambda: t3.decode_frame_async(coded.data_ptr(), n_enc, cfg, n_raw, full.data_ptr(), NPX, ver.data_ptr(), True, s)
    for sub in STD:
        calls["base_window_S%d" % sub] = (lambda sub=sub: base_window(sub))
        calls["base_blit_S%d" % sub] = (lambda sub=sub: t3.blit_center_rgb_dev(src.data_ptr(), STD[sub][0], STD[sub][1], canvas.data_ptr(), FW, FH, s))
if leg in ("new", "both"):
    for sub in STD:
        calls["new_window_S%d" % sub] = (lambda sub=sub: new_window(sub))
        calls["new_compose_S%d" % sub] = (lambda sub=sub: t3.image_compose_dev(src.data_ptr(), STD[sub][0], STD[sub][1], sub, 1, canvas.data_ptr(), s))

for _ in range(200):
    t3.decode_frame_async(coded.data_ptr(), n_enc, cfg, n_raw, full.data_ptr(), NPX, ver.data_ptr(), True, s)
for f in calls.values():
    for _ in range(5): f()
torch.cuda.synchronize()
got = {k: [] for k in calls}
for _ in range(samples):
    for k, f in calls.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n): f()
        e1.record(); torch.cuda.synchronize()
        got[k].append(e0.elapsed_time(e1) / n)
res = {"leg": leg, "lib": "T3HIP_LIB (another build)" if os.environ.get("T3HIP_LIB") else "this tree", "version": t3.version(), "launches": n, "samples": samples, "verdict": ver.cpu().tolist(),
       "ms": {k: float(np.median(v)) for k, v in got.items()}, "ms_min": {k: float(np.min(v)) for k, v in got.items()}}
if leg == "both":   # the two legs' windows agree byte for byte (the last sub-window computed by each)
    base_window(15); new_window(15); torch.cuda.synchronize()
    res["same_bytes"] = bool(torch.equal(rgb_a[: 854 * 480 * 3], rgb_b[: 854 * 480 * 3]))
    res["ratio_new_over_base"] = {"window_S%d" % sub: res["ms"]["new_window_S%d" % sub] / res["ms"]["base_window_S%d" % sub] for sub in STD}
    res["ratio_new_over_base"].update({"compose_S%d" % sub: res["ms"]["new_compose_S%d" % sub] / res["ms"]["base_blit_S%d" % sub] for sub in STD})
line = json.dumps(res)
print(line)
if out_path:
    with open(out_path, "a") as fh:
        fh.write(line + "\n")
