// t3_dec_plan.hpp — the decode side's planner (t3_dec_plan.cpp): the fused FIXED decoder's tile and LDS carve-up, the argument blocks of the
// three FIXED decoders, and the window and repair plans.  Pure C++17, no device: the launch side (t3_api_decode.cpp, t3_api_repair.cpp)
// binds the tables' addresses, the kernel symbol, the caller's pointers and the grid.
#pragma once
#include <stdint.h>

#include <algorithm>

#include "t3_decode.h"
#include "t3_host.hpp"

namespace t3 {

// ---- the fused decoder's geometry (t3_decode_fused.hip and the kernels built from its block stages), defined here once
enum class FusedForm : int { Words = 0, Pixels = 1, Rgb = 2, Repair = 3 };    // the first three: the entry points' to_pixels / out_fmt
constexpr bool fused_px(FusedForm f) { return f == FusedForm::Pixels || f == FusedForm::Rgb; }
constexpr uint32_t kFx2SeqNb = 52u;             // blocks per band and tile of the raw-word and repair kernels (the pixel kernels: T3_DEC_PX_NB)
constexpr uint32_t kFmaBytes = 19696u;          // the multiply-accumulate table [27][27][27], 19683 bytes, in 16-byte granules
constexpr uint32_t kAfragBytes = 3328u;         // room of the A operand of the syndrome MFMA: the kernels stage 3072 bytes (three steps); the 256 behind them
                                                // (a fourth step's row, once) stay unused, so that every planned offset keeps its recorded value -- LDS is
                                                // handed out in 1,280-byte units, and the workgroup needs 42 of them either way
constexpr uint32_t kPatBytes = 192u;            // twelve scrambler pattern rows of 16 bytes
constexpr uint32_t kQEntryBytes = 10u;          // a queue entry: 8 bytes of syndromes + 2 of item number
constexpr uint32_t kUepRecBytes = 128u;         // UEP: group records and pair table
constexpr uint32_t synd_T_bytes(uint32_t copies) { return 3u * 27u * 4u * copies; }
inline uint32_t synd_lut_bytes(int k) { return 26u * (uint32_t)syndrome_lut_slab(k); }     // the two-kernel decoder's syndrome LUT of one k
constexpr uint32_t fused_nb(FusedForm f) { return fused_px(f) ? (uint32_t)T3_DEC_PX_NB : kFx2SeqNb; }
// The tile and its LDS carve-up (layouts: t3_decode.h; repair: the words' without the output stage).  units_tile: pixels, words or (repair) blocks
struct FusedGeom { uint32_t nb, TS, units_tile, fma_off, af_off, pat_off, y_off, y_stride, q_off, q_stride, o_off, lds_bytes; };
FusedGeom fused_geom(int k, FusedForm form);
inline uint32_t fused_tiles(const t3_layout& L, FusedForm form) {
    return (uint32_t)((*std::max_element(L.band_blocks, L.band_blocks + 9) + fused_nb(form) - 1) / fused_nb(form));
}

// il_w, il_A, div_A, div_w of an argument block with the 2-D interleave (rows of tile_w symbols, chunks of tile_w tile_h clamped to n_sym)
template <class A> void fill_interleave(A& a, const t3_cfg& cfg, uint64_t n_sym) {
    a.il_w = cfg.tile_w; a.il_A = (uint32_t)std::min<uint64_t>((uint64_t)cfg.tile_w * cfg.tile_h, n_sym);
    a.div_A = to_dev(fastdiv(a.il_A)); a.div_w = to_dev(fastdiv(a.il_w));
}

// ---- the FIXED decoders, planned: 1 when the framing is not the planner's own, else the argument block filled but for the launch side's
// fields (tables, stream and output pointers, tickets, verdict and header check, edge / ystream) and the kernel named by value.
// body_bytes, hdr_syms: the coded stream and the header symbols in front of its band-serial body.
// Fused decode (t3_decode_fused.hip): one k, 1-D.  bcn_period != 0: the body still carries its beacon symbols (slot bcn_slot of every
// bcn_period-th word, OLD:952-957) and the loads step over them.  tile_lo / tile_hi (pixel forms, no beacon): only that range of tiles --
// the kernel sees a frame of its own, its output out_off bytes behind the frame's; an empty range: T3_E_ARG.  Repair: also 2-D frames.
struct FusedPlan {
    DecFx2Args a; uint64_t out_off; struct { int r; bool px, rgb, bcn; } kern; uint32_t threads; bool tickets, whole_frame;
    const void* fn; uint32_t grid;              // the launch side's
};
int plan_fixed_fused(uint64_t body_bytes, uint32_t hdr_syms, const t3_layout& L, const ScrCycle& sc, uint64_t units, FusedForm form, FusedPlan& p,
                     uint32_t bcn_slot = 0, uint32_t bcn_period = 0, uint32_t tile_lo = 0, uint32_t tile_hi = 0xFFFFFFFFu);
// One launch for per-band k (two codes at most) and / or the 2-D interleave, pixels out (t3_decode_uep.hip): decode_uep_px_kernel<ra, rb>.
// two_kernel: the measurement knob T3HIP_TWO_KERNEL_DECODE
struct UepPlan { DecUepArgs a; int ra, rb; const void* fn; uint32_t grid; };
int plan_fixed_uep(uint64_t body_bytes, uint32_t hdr_syms, const t3_cfg& cfg, const t3_layout& L, const ScrCycle& sc, uint64_t units, bool two_kernel, UepPlan& p);
// Two kernels (t3_decode_stream.hip): any per-band k, 1-D or 2-D.  lut_bytes: the syndrome LUT's size per k index
struct StreamPlan { DecStArgs a; EmitStArgs e; bool to_pixels; const void* emit_fn; uint32_t grid, emit_grid; };
int plan_fixed_stream(uint64_t body_bytes, uint32_t hdr_syms, const t3_cfg& cfg, const t3_layout& L, const ScrCycle& sc, uint64_t units, int to_pixels,
                      const uint32_t lut_bytes[4], StreamPlan& p);

// ---- plans the caller can ask for (t3hip.h).  L: the frame's layout; generic: T3HIP_GENERIC_DECODE is set
// Which tiles of the frame a window's rows live in.  The frame's 2 n_raw pixels are read as rows of fw; the window's pixels are the stream
// pixels [p0, p1) (rows >= fh and pixels behind the stream do not exist and cost nothing).  Tile range: the framing plan_fixed_fused takes
// with a range (FIXED, one k, 1-D, no beacon).  Every other framing: the whole frame, n_tiles = 0.
int plan_window(uint64_t n_raw, const t3_cfg& cfg, uint32_t fw, uint32_t fh, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, bool generic, t3_window_plan& out, t3_layout& L);
// The same window out of every frame of a batch: one frame's window plan, the bytes and stride minima of a frame, and whether the batch is
// one decoder launch over n_frames * (tile_hi - tile_lo) tickets
constexpr uint64_t kWinScratchSlack = 256;      // behind the runs, as the single-frame entry keeps it
int plan_frames_window(uint64_t n_raw, uint32_t n_frames, const t3_cfg& cfg, uint32_t fw, uint32_t fh, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, int out_fmt,
                       bool generic, t3_frames_window_plan& out, t3_layout& L);
// Repair: which kernel serves the framing and over how many tiles; and a batch: one frame's plan P and how the batch runs
constexpr uint32_t kRepairMaxFrames = 65535u;
int plan_repair(uint64_t n_raw, const t3_cfg& cfg, t3_repair_plan& out, t3_layout& L);
int plan_repair_frames(uint64_t n_raw, uint32_t n_frames, const t3_cfg& cfg, t3_repair_frames_plan& out, t3_repair_plan& P, t3_layout& L);
// Decode with erasures (t3hip.h): path 1 exactly where plan_fixed_fused's pixel form serves a frame (one k, 1-D, beacon optional, fmt 1 or 2,
// n_raw > 0), path 0 for everything else the FIXED decoders accept; COMPAT and RAW mode: T3_E_ARG
int plan_decode_erasures(uint64_t n_raw, const t3_cfg& cfg, int fmt, t3_decode_erasures_plan& out, t3_layout& L);
// ... and a path-1 frame's launch: plan_fixed_fused's pixel form on the framed stream of n_in words, its two queues kEraQCap entries each
// (decode_era_px_kernel, t3_decode_era.hip).  1: not a path-1 frame.  tile_lo / tile_hi: plan_fixed_fused's tile range (no beacon)
int plan_fixed_era(uint64_t n_in, const t3_cfg& cfg, const t3_layout& L, const ScrCycle& sc, uint64_t units, int fmt, FusedPlan& p,
                   uint32_t tile_lo = 0, uint32_t tile_hi = 0xFFFFFFFFu);
// ... and a pixel window of such a frame (t3hip.h): the window plan of the same arguments, the erasure plan's path, what the call launches
// (path 1: ONE launch of decode_era_window_px over win's tile range, or over the frame's tiles where there is none -- a beacon, `generic`),
// and whether some window position maps to no stream pixel
int plan_decode_erasures_window(uint64_t n_raw, const t3_cfg& cfg, uint32_t fw, uint32_t fh, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, int out_fmt, bool generic,
                                t3_decode_erasures_window_plan& out, t3_layout& L);

// ... and a batch of equal frames (t3hip.h): one frame's plan, the stride minima, and whether the batch is ONE launch of decode_era_frames_px
// (t3_decode_era_frames.hip) over n_frames * frame.n_tiles tickets -- path 1 and at least two frames -- or a loop of the single-frame body
int plan_decode_erasures_frames(uint64_t n_raw, uint32_t n_frames, const t3_cfg& cfg, int fmt, t3_decode_erasures_frames_plan& out, t3_layout& L);
// ... and the same pixel window out of every frame of such a batch (t3hip.h): one frame's window plan, the stride minima, and whether the
// batch is ONE launch of decode_era_frames_window_px (t3_decode_era_frames_window.hip) over n_frames * frame.tiles_launched tickets -- path
// 1, at least two frames and at least one tile -- or a loop of the single-frame window body
int plan_decode_erasures_frames_window(uint64_t n_raw, uint32_t n_frames, const t3_cfg& cfg, uint32_t fw, uint32_t fh, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, int out_fmt,
                                       bool generic, t3_decode_erasures_frames_window_plan& out, t3_layout& L);

}  // namespace t3
