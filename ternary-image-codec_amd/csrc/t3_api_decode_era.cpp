// t3_api_decode_era.cpp — decode of a FIXED frame with received bytes above 26 taken as erasures, the input read-only (include/t3hip.h,
// "decode with erasures"): the planner's C entry, the asynchronous body decode -- path 1: ONE launch of decode_era_px_kernel
// (t3_decode_era.hip) on the caller's buffer; path 0: a private copy, the erasure repair body on it (repair_body, t3_api_repair.cpp), the
// streaming decoder on the copy -- the synchronous device entry (header parsed on the host) and the host-buffer entry.  Behind them the
// same for a batch of equal frames ("decode with erasures of a batch of equal FIXED frames"): ONE launch of decode_era_frames_px
// (t3_decode_era_frames.hip) over the tile space of all frames where the plan says so, else the single-frame body frame by frame.
// And a pixel window of one frame ("decode a window with erasures"): ONE launch of decode_era_window_px (t3_decode_era_window.hip) over the
// tiles the window covers, which writes the window itself; path 0: the private copy, the repair, the whole-frame window decode of the copy.
// And that window out of every frame of a batch ("decode a window with erasures of a batch of equal FIXED frames"): ONE launch of
// decode_era_frames_window_px (t3_decode_era_frames_window.hip) over the window's tiles of all frames where the plan says so, else the
// single-frame window body frame by frame.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <vector>

#include "../../include/t3hip.h"
#include "t3_ctx.hpp"
#include "t3_dec_plan.hpp"
#include "t3_decode.h"
#include "t3_frame_batch.hpp"
#include "t3_host.hpp"

using namespace t3;

namespace {
constexpr uint64_t kEraWorkBytes = 128;        // behind the private copy: [0, 24) the repair's six words, [32, 36) the decoder's counter, [64, 80) the synchronous entry's verdict
uint64_t unit_bytes(int fmt) { return fmt == 0 ? 9u : fmt == 1 ? 6u : 3u; }
uint64_t era_scratch_bytes(const t3_decode_erasures_plan& P, uint64_t n_in) { return std::max<uint64_t>(P.scratch_bytes, (9 * n_in + 15u) & ~15ull); }

// what a planned frame can be refused for without a device, in the entries' order: arguments, then capacity (then a truncated stream)
int era_check(const void* d_in, uint64_t n_in, const void* d_out, uint64_t cap_units, int fmt, const t3_decode_erasures_plan& P, uint64_t* n_out) {
    if ((n_in && !d_in) || !batch_in_ok(d_in, n_in, 0, 1)) return T3_E_ARG;
    if (P.out_units && !d_out) return T3_E_ARG;
    if (fmt == 1 && ((uintptr_t)d_out & 1u) != 0) return T3_E_ARG;                  // (t3hip_decode_frame_async: 16-bit components)
    if (P.path == 1 && ((uintptr_t)d_out & 15u) != 0) return T3_E_ARG;              // the fused kernel's stores; never silently path 0
    if (cap_units < P.out_units) { *n_out = P.out_units; return T3_E_CAPACITY; }   // (*n_out: what is asked for)
    return T3_OK;
}

// The body of a frame whose configuration is known, all on s.  hx: the expected header symbols (hs of them; null: no compare, word 0 stays 0).
int era_body(const void* d_in, uint64_t n_in, const t3_cfg& cfg, uint64_t n_raw, const t3_layout& L, const t3_decode_erasures_plan& P, const uint8_t next[3],
             void* d_out, int fmt, uint32_t* d_verdict, const HdrExpect* hx, uint32_t hs, hipStream_t s) {
    Ctx& c = ctx();
    if (P.path == 1) {
        if (hs > 96u) return T3_E_ARG;
        const ScrCycle sc = scrambler_cycle_from_next(next, cfg.seed_s0);
        FusedPlan p; { const int rc = plan_fixed_era(n_in, cfg, L, sc, P.out_units, fmt, p); if (rc) return rc < 0 ? rc : T3_E_ARG; }
        const void* fn = by_r(p.kern.r, [&](auto R) -> const void* {
            constexpr int r = decltype(R)::value;
            if (p.kern.rgb) return p.kern.bcn ? (const void*)decode_era_px_kernel<r, true, true> : (const void*)decode_era_px_kernel<r, true, false>;
            return p.kern.bcn ? (const void*)decode_era_px_kernel<r, false, true> : (const void*)decode_era_px_kernel<r, false, false>;
        });
        { const int rc = bind_fused(p, d_out, nullptr, 0, fn); if (rc) return rc; }
        DecFx2Args& a = p.a;
        a.in = (const uint8_t*)d_in; a.verdict = d_verdict; a.hdr_in = (const uint8_t*)d_in; a.hdr_n = hx ? hs : 0u;
        if (hx) memcpy(a.hx, hx->b, 96);
        tile_tickets(c, s, 1, p.grid, &a.tile_ctr, &a.n_classes);
        HIPCHK(hipMemsetAsync(d_verdict, 0, 16, s));
        void* args[] = {(void*)&a};
        HIPCHK(hipLaunchKernel(fn, dim3(p.grid), dim3(p.threads), args, a.lds_bytes, s));
        return T3_OK;
    }
    // path 0: the copy, the erasure repair on it, the plain decoder on the repaired copy; the words are the repair's
    const uint64_t cb = era_scratch_bytes(P, n_in);
    void* d_c; { const int rc = scratch(c, Scratch::StreamErasure, cb + kEraWorkBytes, &d_c, s); if (rc) return rc; }
    uint32_t* const rep6 = (uint32_t*)((uint8_t*)d_c + cb);
    if (n_in) HIPCHK(hipMemcpyAsync(d_c, d_in, 9 * n_in, hipMemcpyDeviceToDevice, s));
    t3_repair_plan rp; t3_layout L2;
    { const int rc = plan_repair(n_raw, cfg, rp, L2); if (rc) return rc; }
    { const int rc = repair_body(d_c, cfg, L, rp, next, T3_REPAIR_WRITE, rep6, hx, hs, s, repair_erasures()); if (rc) return rc; }
    uint64_t n_units = 0;
    { const int rc = decode_body_known(d_c, n_in, cfg, n_raw, next, d_out, P.out_units, &n_units, fmt, rep6 + 8, s); if (rc) return rc < 0 ? rc : T3_E_ARG; }
    hipLaunchKernelGGL(era_verdict_kernel, dim3(1), dim3(64), 0, s, (const uint32_t*)rep6, d_verdict);
    HIPCHK(hipGetLastError());
    return T3_OK;
}

// ---- a batch of equal frames ------------------------------------------------------------------------------------------------------------
// n_frames frames of one known configuration.  Where the plan says one launch (path 1, two frames or more), that or T3_E_ARG, never silently
// a loop: ONE memset of every frame's four verdict words, ONE launch of decode_era_frames_px over the tile space of all frames ([4 f] by that
// launch when `hx` is given).  Else the single-frame body frame by frame on s (the stream's order makes reusing path 0's per-stream scratch
// safe).  hx: the expected header symbols (null: no compare, word 0 stays 0).
int era_frames_run(const void* d_in, uint64_t n_in, uint64_t in_stride, uint32_t n_frames, const t3_cfg& cfg, uint64_t n_raw, const t3_layout& L,
                   const t3_decode_erasures_plan& P, const uint8_t next[3], void* d_out, uint64_t out_stride, int fmt, uint32_t* d_verdict, const HdrExpect* hx, uint32_t hs,
                   hipStream_t s) {
    if (P.path != 1 || n_frames < 2) {
        for (uint32_t f = 0; f < n_frames; ++f) {
            const int rc = era_body((const uint8_t*)d_in + (uint64_t)f * in_stride, n_in, cfg, n_raw, L, P, next, d_out ? (uint8_t*)d_out + (uint64_t)f * out_stride : nullptr, fmt,
                                    d_verdict + 4ull * f, hx, hs, s);
            if (rc) return rc;
        }
        return T3_OK;
    }
    if ((uint64_t)n_frames * P.n_tiles >= (1ull << 31) || hs > 96u) return T3_E_ARG;
    Ctx& c = ctx();
    const ScrCycle sc = scrambler_cycle_from_next(next, cfg.seed_s0);
    // a frame's stream is its L.out_words words, whatever lies behind them in the stride
    FusedPlan p; { const int rc = plan_fixed_era(L.out_words, cfg, L, sc, P.out_units, fmt, p); if (rc) return rc < 0 ? rc : T3_E_ARG; }
    const void* fn = by_r(p.kern.r, [&](auto R) -> const void* {
        constexpr int r = decltype(R)::value;
        if (p.kern.rgb) return p.kern.bcn ? (const void*)decode_era_frames_px<r, true, true> : (const void*)decode_era_frames_px<r, true, false>;
        return p.kern.bcn ? (const void*)decode_era_frames_px<r, false, true> : (const void*)decode_era_frames_px<r, false, false>;
    });
    { const int rc = bind_fused(p, d_out, nullptr, n_frames, fn); if (rc) return rc; }
    if (p.a.n_tiles != P.n_tiles) return T3_E_ARG;
    DecFramesArgs fa; memset(&fa, 0, sizeof fa);
    fa.a = p.a; fa.a.in = (const uint8_t*)d_in; fa.a.verdict = d_verdict; fa.a.hdr_in = (const uint8_t*)d_in; fa.a.hdr_n = hx ? hs : 0u;
    if (hx) memcpy(fa.a.hx, hx->b, 96);
    fa.in_stride = in_stride; fa.out_stride = out_stride; fa.n_frames = n_frames;
    fa.n_total = n_frames * fa.a.n_tiles; fa.div_tiles = to_dev(fastdiv(fa.a.n_tiles));
    tile_tickets(c, s, 1, p.grid, &fa.a.tile_ctr, &fa.a.n_classes);
    HIPCHK(hipMemsetAsync(d_verdict, 0, 16ull * n_frames, s));
    void* args[] = {(void*)&fa};
    HIPCHK(hipLaunchKernel(fn, dim3(p.grid), dim3(p.threads), args, fa.a.lds_bytes, s));
    return T3_OK;
}

// ---- a pixel window of one frame ---------------------------------------------------------------------------------------------------------
struct Window { uint32_t fw, fh, x0, y0, w, h; };
// what a planned window can be refused for without a device (w * h > 0)
int era_win_check(const void* d_in, uint64_t n_in, const void* d_out) {
    return ((n_in && !d_in) || !batch_in_ok(d_in, n_in, 0, 1) || !d_out || ((uintptr_t)d_out & 3u) != 0) ? T3_E_ARG : T3_OK;
}

// The window of a frame whose configuration is known, all on s (w * h > 0).  hx as for era_body.  Nothing is enqueued before the last
// refusal: then the window is zeroed where the plan says so.  Path 1: the verdict words zeroed, ONE launch of decode_era_window_px -- or,
// with no window position in the stream, the header compare alone.  Path 0: era_body's path 0 with the whole-frame window decode
// (decode_window_known: the scrambler as `next`, as the repair takes it -- a parsed header carries the seeds mod 27 only) in the decoder's place.
int era_window_body(const void* d_in, uint64_t n_in, const t3_cfg& cfg, uint64_t n_raw, const t3_layout& L, const t3_decode_erasures_window_plan& P, const uint8_t next[3],
                    const Window& g, void* d_out, int fmt, uint32_t* d_verdict, const HdrExpect* hx, uint32_t hs, hipStream_t s) {
    Ctx& c = ctx();
    const t3_window_plan& wp = P.win;
    if (P.path == 1) {
        if (hs > 96u) return T3_E_ARG;
        if (wp.tile_range && wp.tile_hi == wp.tile_lo) {                           // no tile: the header verdict, zero counts, a zero window
            if (P.zero_fill) HIPCHK(hipMemsetAsync(d_out, 0, P.out_bytes, s));
            HIPCHK(hipMemsetAsync(d_verdict, 0, 16, s));
            if (hx) { hipLaunchKernelGGL(hdr_compare_kernel, dim3(1), dim3(128), 0, s, (const uint8_t*)d_in, *hx, hs, d_verdict); HIPCHK(hipGetLastError()); }
            return T3_OK;
        }
        const ScrCycle sc = scrambler_cycle_from_next(next, cfg.seed_s0);
        const bool range = wp.tile_range && !(wp.tile_lo == 0 && wp.tile_hi == wp.n_tiles);
        FusedPlan p;
        { const int rc = range ? plan_fixed_era(n_in, cfg, L, sc, wp.first_px + wp.n_px, fmt, p, wp.tile_lo, wp.tile_hi) : plan_fixed_era(n_in, cfg, L, sc, 2 * n_raw, fmt, p);
          if (rc) return rc < 0 ? rc : T3_E_ARG; }
        if (p.a.n_tiles != P.tiles_launched) return T3_E_ARG;
        const void* fn = by_r(p.kern.r, [&](auto R) -> const void* {
            constexpr int r = decltype(R)::value;
            if (p.kern.rgb) return p.kern.bcn ? (const void*)decode_era_window_px<r, true, true> : (const void*)decode_era_window_px<r, true, false>;
            return p.kern.bcn ? (const void*)decode_era_window_px<r, false, true> : (const void*)decode_era_window_px<r, false, false>;
        });
        { const int rc = bind_fused(p, d_out, nullptr, 0, fn); if (rc) return rc; }
        DecEraWinArgs wa; memset(&wa, 0, sizeof wa);
        wa.a = p.a;
        DecFx2Args& a = wa.a;
        a.out = d_out;                                                             // the window's first byte, whatever the range's offset in the stream
        a.in = (const uint8_t*)d_in; a.verdict = d_verdict; a.hdr_in = (const uint8_t*)d_in; a.hdr_n = hx ? hs : 0u;
        if (hx) memcpy(a.hx, hx->b, 96);
        wa.fw = g.fw; wa.div_fw = to_dev(fastdiv(g.fw)); wa.x0 = g.x0; wa.y0 = g.y0; wa.w = g.w;
        wa.rows_end = (uint32_t)std::min<uint64_t>((uint64_t)g.y0 + g.h, g.fh);
        wa.first_px = range ? (uint32_t)wp.first_px : 0u; wa.n_px = (uint32_t)(2 * n_raw);   // (9 * out_words < 2^32: the plan)
        tile_tickets(c, s, 1, p.grid, &a.tile_ctr, &a.n_classes);
        if (P.zero_fill) HIPCHK(hipMemsetAsync(d_out, 0, P.out_bytes, s));
        HIPCHK(hipMemsetAsync(d_verdict, 0, 16, s));
        void* args[] = {(void*)&wa};
        HIPCHK(hipLaunchKernel(fn, dim3(p.grid), dim3(p.threads), args, a.lds_bytes, s));
        return T3_OK;
    }
    // path 0: the copy, the erasure repair on it, the whole-frame window decode of the repaired copy (its counter: a work word); the words are the repair's
    const uint64_t cb = (P.in_bytes + 15u) & ~15ull, ccb = std::max<uint64_t>(cb, (9 * n_in + 15u) & ~15ull);
    void* d_c; { const int rc = scratch(c, Scratch::StreamErasure, ccb + kEraWorkBytes, &d_c, s); if (rc) return rc; }
    uint32_t* const rep6 = (uint32_t*)((uint8_t*)d_c + ccb);
    t3_repair_plan rp; t3_layout L2;
    { const int rc = plan_repair(n_raw, cfg, rp, L2); if (rc) return rc; }
    if (P.zero_fill) HIPCHK(hipMemsetAsync(d_out, 0, P.out_bytes, s));
    if (n_in) HIPCHK(hipMemcpyAsync(d_c, d_in, 9 * n_in, hipMemcpyDeviceToDevice, s));
    { const int rc = repair_body(d_c, cfg, L, rp, next, T3_REPAIR_WRITE, rep6, hx, hs, s, repair_erasures()); if (rc) return rc; }
    { const int rc = decode_window_known(d_c, n_in, cfg, n_raw, next, g.fw, g.fh, g.x0, g.y0, g.w, g.h, d_out, fmt, rep6 + 8, s); if (rc) return rc; }
    hipLaunchKernelGGL(era_verdict_kernel, dim3(1), dim3(64), 0, s, (const uint32_t*)rep6, d_verdict);
    HIPCHK(hipGetLastError());
    return T3_OK;
}

// the output of a batch of n_frames >= 2: a 16-byte base, frames a multiple of 16 apart that do not overlap (the input: batch_in_ok)
bool era_out_ok(const void* d_out, uint64_t out_bytes, uint64_t out_stride) {
    return (!out_bytes || d_out) && (((uintptr_t)d_out | out_stride) & 15u) == 0 && out_stride >= out_bytes;
}

// ---- the same pixel window of every frame of a batch -------------------------------------------------------------------------------------
// n_frames frames of one known configuration, the window g of each (w * h > 0).  Where the frame's plan P says so (path 1, two frames or
// more, at least one tile), that or T3_E_ARG, never silently a loop: ONE memset of every frame's four verdict words, ONE 2-D memset of the
// windows where the plan says zero_fill (the stride gaps stay as they are), ONE launch of decode_era_frames_window_px over the tickets of
// all frames ([4 f] by that launch when `hx` is given).  Else the single-frame window body frame by frame on s (the stream's order makes
// reusing path 0's per-stream scratch safe).  Nothing is enqueued before the last refusal.
int era_frames_window_run(const void* d_in, uint64_t n_in, uint64_t in_stride, uint32_t n_frames, const t3_cfg& cfg, uint64_t n_raw, const t3_layout& L,
                          const t3_decode_erasures_window_plan& P, const uint8_t next[3], const Window& g, void* d_out, uint64_t out_stride, int fmt, uint32_t* d_verdict,
                          const HdrExpect* hx, uint32_t hs, hipStream_t s) {
    if (P.path != 1 || n_frames < 2 || P.tiles_launched == 0) {
        for (uint32_t f = 0; f < n_frames; ++f) {
            const int rc = era_window_body((const uint8_t*)d_in + (uint64_t)f * in_stride, n_in, cfg, n_raw, L, P, next, g, (uint8_t*)d_out + (uint64_t)f * out_stride, fmt,
                                           d_verdict + 4ull * f, hx, hs, s);
            if (rc) return rc;
        }
        return T3_OK;
    }
    if ((uint64_t)n_frames * P.tiles_launched >= (1ull << 31) || hs > 96u) return T3_E_ARG;
    Ctx& c = ctx();
    const t3_window_plan& wp = P.win;
    const ScrCycle sc = scrambler_cycle_from_next(next, cfg.seed_s0);
    const bool range = wp.tile_range && !(wp.tile_lo == 0 && wp.tile_hi == wp.n_tiles);      // (era_window_body's choice)
    // a frame's stream is its L.out_words words, whatever lies behind them in the stride
    FusedPlan p;
    { const int rc = range ? plan_fixed_era(L.out_words, cfg, L, sc, wp.first_px + wp.n_px, fmt, p, wp.tile_lo, wp.tile_hi) : plan_fixed_era(L.out_words, cfg, L, sc, 2 * n_raw, fmt, p);
      if (rc) return rc < 0 ? rc : T3_E_ARG; }
    const void* fn = by_r(p.kern.r, [&](auto R) -> const void* {
        constexpr int r = decltype(R)::value;
        if (p.kern.rgb) return p.kern.bcn ? (const void*)decode_era_frames_window_px<r, true, true> : (const void*)decode_era_frames_window_px<r, true, false>;
        return p.kern.bcn ? (const void*)decode_era_frames_window_px<r, false, true> : (const void*)decode_era_frames_window_px<r, false, false>;
    });
    { const int rc = bind_fused(p, d_out, nullptr, n_frames, fn); if (rc) return rc; }
    if (p.a.n_tiles != P.tiles_launched) return T3_E_ARG;
    DecEraWinFramesArgs fa; memset(&fa, 0, sizeof fa);
    DecEraWinArgs& wa = fa.w;
    wa.a = p.a;
    DecFx2Args& a = wa.a;
    a.out = d_out;                                                                 // frame 0's window, whatever the range's offset in the stream
    a.in = (const uint8_t*)d_in; a.verdict = d_verdict; a.hdr_in = (const uint8_t*)d_in; a.hdr_n = hx ? hs : 0u;
    if (hx) memcpy(a.hx, hx->b, 96);
    wa.fw = g.fw; wa.div_fw = to_dev(fastdiv(g.fw)); wa.x0 = g.x0; wa.y0 = g.y0; wa.w = g.w;
    wa.rows_end = (uint32_t)std::min<uint64_t>((uint64_t)g.y0 + g.h, g.fh);
    wa.first_px = range ? (uint32_t)wp.first_px : 0u; wa.n_px = (uint32_t)(2 * n_raw);       // (9 * out_words < 2^32: the plan)
    fa.in_stride = in_stride; fa.out_stride = out_stride; fa.n_frames = n_frames;
    fa.n_total = n_frames * a.n_tiles; fa.div_tiles = to_dev(fastdiv(a.n_tiles));
    tile_tickets(c, s, 1, p.grid, &a.tile_ctr, &a.n_classes);
    HIPCHK(hipMemsetAsync(d_verdict, 0, 16ull * n_frames, s));
    if (P.zero_fill) HIPCHK(hipMemset2DAsync(d_out, out_stride, 0, P.out_bytes, n_frames, s));
    void* args[] = {(void*)&fa};
    HIPCHK(hipLaunchKernel(fn, dim3(p.grid), dim3(p.threads), args, a.lds_bytes, s));
    return T3_OK;
}
}  // namespace

extern "C" {

int t3hip_decode_erasures_plan(uint64_t n_raw, const t3_cfg* cfg, int fmt, t3_decode_erasures_plan* out) {
    if (!cfg || !out) return T3_E_ARG;
    t3_layout L;
    return plan_decode_erasures(n_raw, *cfg, fmt, *out, L);
}

int t3hip_decode_erasures_frame_async(const void* d_in, uint64_t n_in, const t3_cfg* cfg, uint64_t n_raw, void* d_out, uint64_t cap_units, uint64_t* n_out, int fmt,
                                      uint32_t* d_verdict, void* stream) {
    // what can be refused without a device is refused first
    if (!cfg || !n_out || !d_verdict) return T3_E_ARG;
    t3_decode_erasures_plan P; t3_layout L;
    { const int rc = plan_decode_erasures(n_raw, *cfg, fmt, P, L); if (rc) return rc; }
    *n_out = P.out_units;
    { const int rc = era_check(d_in, n_in, d_out, cap_units, fmt, P, n_out); if (rc) return rc; }
    if (L.out_words > n_in) return T3_E_HEADER;                                    // truncated stream
    if (!ctx().ready) return T3_E_NODEVICE;
    const KnownFrame k = known_frame(*cfg, n_raw);
    return era_body(d_in, n_in, *cfg, n_raw, L, P, k.next, d_out, fmt, d_verdict, &k.hx, k.hs, (hipStream_t)stream);
}

int t3hip_decode_erasures_profile_dev(const void* d_in, uint64_t n_in, t3_cfg* seen, void* d_out, uint64_t cap_units, uint64_t* n_out, int fmt, uint32_t counts[4],
                                      void* stream) {
    if (!seen || !n_out || !counts || (n_in && !d_in) || ((uintptr_t)d_in & 1u) != 0 || fmt < 0 || fmt > 2) return T3_E_ARG;
    if (seen->mode != T3_MODE_FIXED || seen->profile == T3_RAW_MODE) return T3_E_ARG;
    Ctx& c = ctx(); if (!c.ready) return T3_E_NODEVICE;
    memset(counts, 0, 4 * sizeof(uint32_t)); *n_out = 0;
    hipStream_t s = (hipStream_t)stream;
    if (n_in < 10) return T3_E_HEADER;
    uint8_t got[90];
    { const int rc = fetch_headers(got, d_in, 90, 1, s); if (rc) return rc; }
    FrameHeader h; t3_decode_erasures_plan P; t3_layout L;
    { const int rc = accept_header(got, n_in, *seen, h, L, [&](uint64_t n_raw, const t3_cfg& cfg, t3_layout& l) {
          const int rc = plan_decode_erasures(n_raw, cfg, fmt, P, l);              // (T3_E_ARG: a header that names a framing nobody encodes)
          return rc ? (rc == T3_E_ARG ? T3_E_HEADER : rc) : era_check(d_in, n_in, d_out, cap_units, fmt, P, n_out); });
      if (rc) return rc; }
    *seen = h.cfg;                                                                 // the header decoded (OLD:1006-1013)
    const uint64_t cb = P.path == 1 ? 0 : era_scratch_bytes(P, n_in);              // (path 0 asks for the same bytes: the scratch does not move)
    void* d_w; { const int rc = scratch(c, Scratch::StreamErasure, cb + kEraWorkBytes, &d_w, s); if (rc) return rc; }
    uint32_t* const d_v = (uint32_t*)((uint8_t*)d_w + cb + 64);
    { const int rc = era_body(d_in, n_in, h.cfg, h.n_raw, L, P, h.next, d_out, fmt, d_v, nullptr, 0, s); if (rc) return rc; }
    int frc; { const int rc = fetch_verdicts(d_v, 4, 1, nullptr, counts, &frc, s); if (rc) return rc; }
    *n_out = P.out_units;
    return frc;
}

int t3hip_decode_erasures_profile(const void* in9, uint64_t n_in, t3_cfg* seen, void* out, uint64_t cap_units, uint64_t* n_out, int fmt, uint32_t counts[4]) {
    if (!seen || !n_out || !counts || (n_in && !in9) || fmt < 0 || fmt > 2 || n_in > (1ull << 40)) return T3_E_ARG;
    if (seen->mode != T3_MODE_FIXED || seen->profile == T3_RAW_MODE) return T3_E_ARG;
    Ctx& c = ctx(); if (!c.ready) return T3_E_NODEVICE;
    std::lock_guard<std::recursive_mutex> hl(c.host_mu);                           // one caller at a time on the shared stream and scratch
    // a frame of n_in coded words holds fewer raw words than that: the output staging never exceeds 2 n_in units
    const uint64_t stage_units = std::min<uint64_t>(cap_units, 2 * n_in);
    void *di, *dout; { const int rc = host_stage(c, in9, 9 * n_in, &di, stage_units * unit_bytes(fmt), &dout); if (rc) return rc; }
    const int rc = t3hip_decode_erasures_profile_dev(di, n_in, seen, out ? dout : nullptr, stage_units, n_out, fmt, counts, c.stream);
    if (rc != T3_OK && rc != T3_E_RS) return rc;
    if (*n_out) { const int frc = host_fetch(c, out, dout, *n_out * unit_bytes(fmt)); if (frc) return frc; }
    return rc;
}

// ---- a batch of equal frames (t3hip.h) --------------------------------------------------------------------------------------------------
int t3hip_decode_erasures_frames_plan(uint64_t n_raw, uint32_t n_frames, const t3_cfg* cfg, int fmt, t3_decode_erasures_frames_plan* out) {
    if (!cfg || !out) return T3_E_ARG;
    t3_layout L;
    return plan_decode_erasures_frames(n_raw, n_frames, *cfg, fmt, *out, L);
}

int t3hip_decode_erasures_frames_async(const void* d_in, uint64_t n_in, uint64_t in_stride, uint32_t n_frames, const t3_cfg* cfg, uint64_t n_raw, void* d_out,
                                       uint64_t out_stride, int fmt, uint32_t* d_verdict, void* stream) {
    if (n_frames == 0) return T3_OK;                                               // nothing launched, nothing written, null pointers allowed
    // what can be refused without a device is refused first
    if (!cfg || !d_verdict) return T3_E_ARG;
    t3_decode_erasures_frames_plan FP; t3_layout L;
    { const int rc = plan_decode_erasures_frames(n_raw, n_frames, *cfg, fmt, FP, L); if (rc) return rc; }
    const t3_decode_erasures_plan& P = FP.frame;
    if (n_frames == 1) { uint64_t n = 0; return t3hip_decode_erasures_frame_async(d_in, n_in, cfg, n_raw, d_out, P.out_units, &n, fmt, d_verdict, stream); }
    if ((n_in && !d_in) || !batch_in_ok(d_in, n_in, in_stride, n_frames) || !era_out_ok(d_out, FP.out_bytes, out_stride) || out_stride < FP.out_stride_min) return T3_E_ARG;
    if (L.out_words > n_in) return T3_E_HEADER;                                    // truncated streams
    if (!ctx().ready) return T3_E_NODEVICE;
    const KnownFrame k = known_frame(*cfg, n_raw);
    return era_frames_run(d_in, n_in, in_stride, n_frames, *cfg, n_raw, L, P, k.next, d_out, out_stride, fmt, d_verdict, &k.hx, k.hs, (hipStream_t)stream);
}

int t3hip_decode_erasures_frames_dev(const void* d_in, uint64_t n_in, uint64_t in_stride, uint32_t n_frames, t3_cfg* seen, void* d_out, uint64_t out_stride,
                                     uint64_t cap_units, uint64_t* n_out, int fmt, uint32_t* counts, int* frame_rc, void* stream) {
    if (n_frames == 0) { if (n_out) *n_out = 0; return T3_OK; }
    if (!seen || !n_out || !counts || !frame_rc || fmt < 0 || fmt > 2 || n_frames > kRepairMaxFrames) return T3_E_ARG;
    const uint64_t UB = unit_bytes(fmt);
    if ((n_in && !d_in) || !batch_in_ok(d_in, n_in, in_stride, n_frames) || cap_units > (~0ull) / 9 || (cap_units && !d_out)) return T3_E_ARG;
    if (n_frames > 1 && !era_out_ok(d_out, cap_units * UB, out_stride)) return T3_E_ARG;
    if (seen->mode != T3_MODE_FIXED || seen->profile == T3_RAW_MODE) return T3_E_ARG;
    if (n_in < 10) return T3_E_HEADER;                                             // no room for a header: nothing decodes
    Ctx& c = ctx(); if (!c.ready) return T3_E_NODEVICE;
    memset(counts, 0, 4ull * n_frames * sizeof(uint32_t)); *n_out = 0;
    for (uint32_t f = 0; f < n_frames; ++f) frame_rc[f] = T3_E_HEADER;
    hipStream_t s = (hipStream_t)stream;
    if (n_frames == 1) {                                                           // the single-frame entry, its output rule
        const int rc = t3hip_decode_erasures_profile_dev(d_in, n_in, seen, d_out, cap_units, n_out, fmt, counts, stream);
        if (rc != T3_OK && rc != T3_E_RS && rc != T3_E_CAPACITY) return rc;
        frame_rc[0] = rc;
        return T3_OK;
    }
    std::vector<uint8_t> got(90ull * n_frames), go(n_frames);                      // go: frames whose body is decoded
    { const int rc = fetch_headers(got.data(), d_in, in_stride, n_frames, s); if (rc) return rc; }
    std::vector<FrameHeader> hd(n_frames); std::vector<t3_decode_erasures_plan> P(n_frames); std::vector<t3_layout> L(n_frames); std::vector<uint64_t> units(n_frames);
    if (!parse_headers(got.data(), n_frames, n_in, seen, hd.data(), L.data(), go.data(), [&](uint32_t f, uint64_t n_raw, const t3_cfg& cfg, t3_layout& l) {
            const int rc = plan_decode_erasures(n_raw, cfg, fmt, P[f], l); units[f] = P[f].out_units; return rc; }))
        return T3_E_HEADER;
    *n_out = select_equal_frames(units.data(), n_frames, cap_units, go.data(), frame_rc);
    void* d_v; { const int rc = scratch(c, Scratch::StreamEraVerdict, 16ull * n_frames + 64, &d_v, s); if (rc) return rc; }
    for (uint32_t f0 = 0, f1 = 0; next_run(go.data(), hd.data(), n_frames, f1, &f0, &f1);) {      // one batched body decode each
        const FrameHeader& h = hd[f0];
        const int rc = era_frames_run((const uint8_t*)d_in + (uint64_t)f0 * in_stride, n_in, in_stride, f1 - f0, h.cfg, h.n_raw, L[f0], P[f0], h.next,
                                      d_out ? (uint8_t*)d_out + (uint64_t)f0 * out_stride : nullptr, out_stride, fmt, (uint32_t*)d_v + 4ull * f0, nullptr, 0, s);
        if (rc) return rc;
    }
    return fetch_verdicts(d_v, 4, n_frames, go.data(), counts, frame_rc, s);
}

int t3hip_decode_erasures_frames(const void* in9, uint64_t n_in, uint64_t in_stride, uint32_t n_frames, t3_cfg* seen, void* out, uint64_t out_stride, uint64_t cap_units,
                                 uint64_t* n_out, int fmt, uint32_t* counts, int* frame_rc) {
    if (n_frames == 0) { if (n_out) *n_out = 0; return T3_OK; }
    if (!seen || !n_out || !counts || !frame_rc || fmt < 0 || fmt > 2 || n_frames > kRepairMaxFrames || n_in > (1ull << 40)) return T3_E_ARG;
    const uint64_t UB = unit_bytes(fmt);
    if ((n_in && !in9) || (cap_units && !out) || (n_frames > 1 && (in_stride < 9 * n_in || out_stride / UB < cap_units))) return T3_E_ARG;
    if (seen->mode != T3_MODE_FIXED || seen->profile == T3_RAW_MODE) return T3_E_ARG;
    if (n_in < 10) return T3_E_HEADER;
    Ctx& c = ctx(); if (!c.ready) return T3_E_NODEVICE;
    std::lock_guard<std::recursive_mutex> hl(c.host_mu);                           // one caller at a time on the shared stream and scratch
    // on the device the frames lie strides of their own apart: only the frames' 9 * n_in bytes travel up, only the output spans down.
    // A frame of n_in coded words holds fewer raw words than that: the output staging never exceeds 2 n_in units a frame
    const uint64_t stage_units = std::min<uint64_t>(cap_units, 2 * n_in);
    const FrameStage g = frame_stage(n_in, in_stride, n_frames);
    const uint64_t dos = (stage_units * UB + 15u) & ~15ull, hos = n_frames > 1 ? out_stride : stage_units * UB;
    void *di, *dout;
    { const int rc = scratch(c, Scratch::HostIn, (size_t)(g.dev_stride * n_frames + 64), &di); if (rc) return rc; }
    { const int rc = scratch(c, Scratch::HostOut, (size_t)(dos * n_frames + 64), &dout); if (rc) return rc; }
    hipStream_t s = c.stream;
    HIPCHK(hipMemcpy2DAsync(di, g.dev_stride, in9, g.pitch, g.bytes, n_frames, hipMemcpyHostToDevice, s));
    const int rc = t3hip_decode_erasures_frames_dev(di, n_in, g.dev_stride, n_frames, seen, dout, dos, stage_units, n_out, fmt, counts, frame_rc, s);
    if (rc != T3_OK) return rc;
    const uint64_t ob = *n_out * UB;
    std::vector<uint8_t> done(n_frames);
    for (uint32_t f = 0; f < n_frames; ++f) done[f] = frame_rc[f] == T3_OK || frame_rc[f] == T3_E_RS;
    for (uint32_t f0 = 0, f1 = 0; ob && next_run(done.data(), nullptr, n_frames, f1, &f0, &f1);)      // the output spans of the decoded frames: one copy per run of them
        HIPCHK(hipMemcpy2DAsync((uint8_t*)out + (uint64_t)f0 * hos, hos, (const uint8_t*)dout + (uint64_t)f0 * dos, dos, ob, f1 - f0, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return T3_OK;
}

// ---- a pixel window of one frame (t3hip.h) ----------------------------------------------------------------------------------------------
int t3hip_decode_erasures_window_plan(uint64_t n_raw, const t3_cfg* cfg, uint32_t fw, uint32_t fh, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, int out_fmt,
                                      t3_decode_erasures_window_plan* out) {
    if (!cfg || !out) return T3_E_ARG;
    t3_layout L;
    return plan_decode_erasures_window(n_raw, *cfg, fw, fh, x0, y0, w, h, out_fmt, generic_decode(), *out, L);
}

int t3hip_decode_erasures_window_async(const void* d_in, uint64_t n_in, const t3_cfg* cfg, uint64_t n_raw, uint32_t fw, uint32_t fh, uint32_t x0, uint32_t y0, uint32_t w,
                                       uint32_t h, void* d_out, int out_fmt, uint32_t* d_verdict, void* stream) {
    // what can be refused without a device is refused first
    if (!cfg || !d_verdict) return T3_E_ARG;
    t3_decode_erasures_window_plan P; t3_layout L;
    { const int rc = plan_decode_erasures_window(n_raw, *cfg, fw, fh, x0, y0, w, h, out_fmt, generic_decode(), P, L); if (rc) return rc; }
    if (P.out_bytes == 0) return T3_OK;                                            // nothing launched, d_verdict untouched
    { const int rc = era_win_check(d_in, n_in, d_out); if (rc) return rc; }
    if (L.out_words > n_in) return T3_E_HEADER;                                    // truncated stream
    if (!ctx().ready) return T3_E_NODEVICE;
    const KnownFrame k = known_frame(*cfg, n_raw);
    return era_window_body(d_in, n_in, *cfg, n_raw, L, P, k.next, Window{fw, fh, x0, y0, w, h}, d_out, out_fmt, d_verdict, &k.hx, k.hs, (hipStream_t)stream);
}

int t3hip_decode_erasures_window_dev(const void* d_in, uint64_t n_in, t3_cfg* seen, uint32_t fw, uint32_t fh, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, void* d_out,
                                     int out_fmt, uint32_t counts[4], void* stream) {
    if (!seen || !counts || (n_in && !d_in) || ((uintptr_t)d_in & 1u) != 0 || (out_fmt != 1 && out_fmt != 2) || fw == 0 || (uint64_t)x0 + w > fw) return T3_E_ARG;
    if (seen->mode != T3_MODE_FIXED || seen->profile == T3_RAW_MODE) return T3_E_ARG;
    const bool empty = (uint64_t)w * h == 0;
    if (!empty && era_win_check(d_in, n_in, d_out) != T3_OK) return T3_E_ARG;
    Ctx& c = ctx(); if (!c.ready) return T3_E_NODEVICE;
    memset(counts, 0, 4 * sizeof(uint32_t));
    hipStream_t s = (hipStream_t)stream;
    if (n_in < 10) return T3_E_HEADER;
    uint8_t got[90];
    { const int rc = fetch_headers(got, d_in, 90, 1, s); if (rc) return rc; }
    FrameHeader hd; t3_decode_erasures_window_plan P; t3_layout L;
    { const int rc = accept_header(got, n_in, *seen, hd, L, [&](uint64_t n_raw, const t3_cfg& cfg, t3_layout& l) {
          const int rc = plan_decode_erasures_window(n_raw, cfg, fw, fh, x0, y0, w, h, out_fmt, generic_decode(), P, l);
          return rc == T3_E_ARG ? T3_E_HEADER : rc; });                            // (the window's own refusals stand above: a header that names a framing nobody encodes)
      if (rc) return rc; }
    *seen = hd.cfg;                                                                // the header decoded (OLD:1006-1013)
    if (empty) return T3_OK;
    const uint64_t cb = P.path == 1 ? 0 : std::max<uint64_t>((P.in_bytes + 15u) & ~15ull, (9 * n_in + 15u) & ~15ull);   // (path 0 asks for the same bytes: the scratch does not move)
    void* d_w; { const int rc = scratch(c, Scratch::StreamErasure, cb + kEraWorkBytes, &d_w, s); if (rc) return rc; }
    uint32_t* const d_v = (uint32_t*)((uint8_t*)d_w + cb + 64);
    { const int rc = era_window_body(d_in, n_in, hd.cfg, hd.n_raw, L, P, hd.next, Window{fw, fh, x0, y0, w, h}, d_out, out_fmt, d_v, nullptr, 0, s); if (rc) return rc; }
    int frc; { const int rc = fetch_verdicts(d_v, 4, 1, nullptr, counts, &frc, s); if (rc) return rc; }
    return frc;
}

int t3hip_decode_erasures_window(const void* in9, uint64_t n_in, t3_cfg* seen, uint32_t fw, uint32_t fh, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, void* out, int out_fmt,
                                 uint32_t counts[4]) {
    if (!seen || !counts || (n_in && !in9) || (out_fmt != 1 && out_fmt != 2) || n_in > (1ull << 40) || fw == 0 || (uint64_t)x0 + w > fw) return T3_E_ARG;
    if (seen->mode != T3_MODE_FIXED || seen->profile == T3_RAW_MODE) return T3_E_ARG;
    const uint64_t out_bytes = (uint64_t)w * h * (out_fmt == 2 ? 3u : 6u);
    if (out_bytes && !out) return T3_E_ARG;
    Ctx& c = ctx(); if (!c.ready) return T3_E_NODEVICE;
    std::lock_guard<std::recursive_mutex> hl(c.host_mu);                           // one caller at a time on the shared stream and scratch
    void *di, *dout; { const int rc = host_stage(c, in9, 9 * n_in, &di, out_bytes, &dout); if (rc) return rc; }
    const int rc = t3hip_decode_erasures_window_dev(di, n_in, seen, fw, fh, x0, y0, w, h, dout, out_fmt, counts, c.stream);
    if (rc != T3_OK && rc != T3_E_RS) return rc;
    if (out_bytes) { const int frc = host_fetch(c, out, dout, out_bytes); if (frc) return frc; }
    return rc;
}

// ---- the same pixel window of every frame of a batch (t3hip.h) ---------------------------------------------------------------------------
int t3hip_decode_erasures_frames_window_plan(uint64_t n_raw, uint32_t n_frames, const t3_cfg* cfg, uint32_t fw, uint32_t fh, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                                             int out_fmt, t3_decode_erasures_frames_window_plan* out) {
    if (!cfg || !out) return T3_E_ARG;
    t3_layout L;
    return plan_decode_erasures_frames_window(n_raw, n_frames, *cfg, fw, fh, x0, y0, w, h, out_fmt, generic_decode(), *out, L);
}

int t3hip_decode_erasures_frames_window_async(const void* d_in, uint64_t n_in, uint64_t in_stride, uint32_t n_frames, const t3_cfg* cfg, uint64_t n_raw, uint32_t fw, uint32_t fh,
                                              uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, void* d_out, uint64_t out_stride, int out_fmt, uint32_t* d_verdict, void* stream) {
    if (n_frames == 0) return T3_OK;                                               // nothing launched, nothing written, null pointers allowed
    // what can be refused without a device is refused first
    if (!cfg || !d_verdict) return T3_E_ARG;
    t3_decode_erasures_frames_window_plan FP; t3_layout L;
    { const int rc = plan_decode_erasures_frames_window(n_raw, n_frames, *cfg, fw, fh, x0, y0, w, h, out_fmt, generic_decode(), FP, L); if (rc) return rc; }
    if (FP.out_bytes == 0) return T3_OK;                                           // nothing launched, d_verdict untouched
    if (n_frames == 1) return t3hip_decode_erasures_window_async(d_in, n_in, cfg, n_raw, fw, fh, x0, y0, w, h, d_out, out_fmt, d_verdict, stream);
    if ((n_in && !d_in) || !batch_in_ok(d_in, n_in, in_stride, n_frames) || !era_out_ok(d_out, FP.out_bytes, out_stride) || out_stride < FP.out_stride_min) return T3_E_ARG;
    if (L.out_words > n_in) return T3_E_HEADER;                                    // truncated streams
    if (!ctx().ready) return T3_E_NODEVICE;
    const KnownFrame k = known_frame(*cfg, n_raw);
    return era_frames_window_run(d_in, n_in, in_stride, n_frames, *cfg, n_raw, L, FP.frame, k.next, Window{fw, fh, x0, y0, w, h}, d_out, out_stride, out_fmt, d_verdict, &k.hx, k.hs,
                                 (hipStream_t)stream);
}

int t3hip_decode_erasures_frames_window_dev(const void* d_in, uint64_t n_in, uint64_t in_stride, uint32_t n_frames, t3_cfg* seen, uint32_t fw, uint32_t fh, uint32_t x0, uint32_t y0,
                                            uint32_t w, uint32_t h, void* d_out, uint64_t out_stride, int out_fmt, uint32_t* counts, int* frame_rc, void* stream) {
    if (n_frames == 0) return T3_OK;
    if (!seen || !counts || !frame_rc || (out_fmt != 1 && out_fmt != 2) || fw == 0 || (uint64_t)x0 + w > fw || n_frames > kRepairMaxFrames) return T3_E_ARG;
    if ((n_in && !d_in) || !batch_in_ok(d_in, n_in, in_stride, n_frames)) return T3_E_ARG;
    const uint64_t out_bytes = (uint64_t)w * h * (out_fmt == 2 ? 3u : 6u);
    const bool empty = out_bytes == 0;
    if (!empty && (n_frames > 1 ? !era_out_ok(d_out, out_bytes, out_stride) : era_win_check(d_in, n_in, d_out) != T3_OK)) return T3_E_ARG;
    if (seen->mode != T3_MODE_FIXED || seen->profile == T3_RAW_MODE) return T3_E_ARG;
    if (n_in < 10) return T3_E_HEADER;                                             // no room for a header: nothing decodes
    Ctx& c = ctx(); if (!c.ready) return T3_E_NODEVICE;
    memset(counts, 0, 4ull * n_frames * sizeof(uint32_t));
    for (uint32_t f = 0; f < n_frames; ++f) frame_rc[f] = T3_E_HEADER;
    hipStream_t s = (hipStream_t)stream;
    if (n_frames == 1) {                                                           // the single-frame entry, its output rule
        const int rc = t3hip_decode_erasures_window_dev(d_in, n_in, seen, fw, fh, x0, y0, w, h, d_out, out_fmt, counts, stream);
        if (rc != T3_OK && rc != T3_E_RS) return rc;
        frame_rc[0] = rc;
        return T3_OK;
    }
    std::vector<uint8_t> got(90ull * n_frames), go(n_frames);                      // go: frames whose body is decoded
    { const int rc = fetch_headers(got.data(), d_in, in_stride, n_frames, s); if (rc) return rc; }
    std::vector<FrameHeader> hd(n_frames); std::vector<t3_decode_erasures_window_plan> P(n_frames); std::vector<t3_layout> L(n_frames);
    if (!parse_headers(got.data(), n_frames, n_in, seen, hd.data(), L.data(), go.data(), [&](uint32_t f, uint64_t n_raw, const t3_cfg& cfg, t3_layout& l) {
            return plan_decode_erasures_window(n_raw, cfg, fw, fh, x0, y0, w, h, out_fmt, generic_decode(), P[f], l); }))
        return T3_E_HEADER;
    if (empty) {                                                                   // nothing is launched: the headers' verdict alone
        for (uint32_t f = 0; f < n_frames; ++f) if (go[f]) frame_rc[f] = T3_OK;
        return T3_OK;
    }
    void* d_v; { const int rc = scratch(c, Scratch::StreamEraVerdict, 16ull * n_frames + 64, &d_v, s); if (rc) return rc; }
    for (uint32_t f0 = 0, f1 = 0; next_run(go.data(), hd.data(), n_frames, f1, &f0, &f1);) {      // one batched body each
        const FrameHeader& h0 = hd[f0];
        const int rc = era_frames_window_run((const uint8_t*)d_in + (uint64_t)f0 * in_stride, n_in, in_stride, f1 - f0, h0.cfg, h0.n_raw, L[f0], P[f0], h0.next,
                                             Window{fw, fh, x0, y0, w, h}, (uint8_t*)d_out + (uint64_t)f0 * out_stride, out_stride, out_fmt, (uint32_t*)d_v + 4ull * f0, nullptr, 0, s);
        if (rc) return rc;
    }
    return fetch_verdicts(d_v, 4, n_frames, go.data(), counts, frame_rc, s);
}

int t3hip_decode_erasures_frames_window(const void* in9, uint64_t n_in, uint64_t in_stride, uint32_t n_frames, t3_cfg* seen, uint32_t fw, uint32_t fh, uint32_t x0, uint32_t y0,
                                        uint32_t w, uint32_t h, void* out, uint64_t out_stride, int out_fmt, uint32_t* counts, int* frame_rc) {
    if (n_frames == 0) return T3_OK;
    if (!seen || !counts || !frame_rc || (out_fmt != 1 && out_fmt != 2) || fw == 0 || (uint64_t)x0 + w > fw || n_frames > kRepairMaxFrames || n_in > (1ull << 40)) return T3_E_ARG;
    const uint64_t out_bytes = (uint64_t)w * h * (out_fmt == 2 ? 3u : 6u);
    if ((n_in && !in9) || (out_bytes && !out) || (n_frames > 1 && (in_stride < 9 * n_in || out_stride < out_bytes))) return T3_E_ARG;
    if (seen->mode != T3_MODE_FIXED || seen->profile == T3_RAW_MODE) return T3_E_ARG;
    if (n_in < 10) return T3_E_HEADER;
    Ctx& c = ctx(); if (!c.ready) return T3_E_NODEVICE;
    std::lock_guard<std::recursive_mutex> hl(c.host_mu);                           // one caller at a time on the shared stream and scratch
    // on the device the frames lie strides of their own apart: only the frames' 9 * n_in bytes travel up, only the windows down
    const FrameStage g = frame_stage(n_in, in_stride, n_frames);
    const uint64_t dos = (out_bytes + 15u) & ~15ull, hos = n_frames > 1 ? out_stride : out_bytes;
    void *di, *dout;
    { const int rc = scratch(c, Scratch::HostIn, (size_t)(g.dev_stride * n_frames + 64), &di); if (rc) return rc; }
    { const int rc = scratch(c, Scratch::HostOut, (size_t)(dos * n_frames + 64), &dout); if (rc) return rc; }
    hipStream_t s = c.stream;
    HIPCHK(hipMemcpy2DAsync(di, g.dev_stride, in9, g.pitch, g.bytes, n_frames, hipMemcpyHostToDevice, s));
    const int rc = t3hip_decode_erasures_frames_window_dev(di, n_in, g.dev_stride, n_frames, seen, fw, fh, x0, y0, w, h, dout, dos, out_fmt, counts, frame_rc, s);
    if (rc != T3_OK) return rc;
    std::vector<uint8_t> done(n_frames);
    for (uint32_t f = 0; f < n_frames; ++f) done[f] = frame_rc[f] == T3_OK || frame_rc[f] == T3_E_RS;
    for (uint32_t f0 = 0, f1 = 0; out_bytes && next_run(done.data(), nullptr, n_frames, f1, &f0, &f1);)      // the windows of the decoded frames: one copy per run of them
        HIPCHK(hipMemcpy2DAsync((uint8_t*)out + (uint64_t)f0 * hos, hos, (const uint8_t*)dout + (uint64_t)f0 * dos, dos, out_bytes, f1 - f0, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return T3_OK;
}

}  // extern "C"
