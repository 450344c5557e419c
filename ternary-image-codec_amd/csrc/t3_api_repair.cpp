// t3_api_repair.cpp — repair of a FIXED coded frame in place (include/t3hip.h, "repair"): the planner, the launcher of the two kernels
// of t3_repair.hip, the synchronous device entry (header parsed and repaired on the host) and the host-buffer entry; and the same four
// for a batch of equal frames, whose bodies go through ONE launch of repair_frames_kernel (t3_repair_frames.hip) where the fused kernel
// serves a frame.  Every one of them also with received bytes above 26 taken as erasures (kErasures: t3_repair_era.hip,
// t3_repair_era_frames.hip).  What the entries decide on the host about headers, runs, addresses and verdicts: t3_frame_batch.hpp.
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
#include "t3_repair.h"

using namespace t3;

namespace {
// the bytes behind the last body symbol up to the frame's last word, and the beacon slot that may sit among them
void fill_edge(RepairEdge& e, const t3_cfg& cfg, const t3_layout& L, void* d_io, uint32_t flags, uint32_t* d_verdict) {
    e.io = (uint8_t*)d_io; e.verdict = d_verdict; e.write = (flags & T3_REPAIR_WRITE) ? 1u : 0u;
    const uint64_t B = L.body_syms;
    uint64_t next = B; e.tail_skip = 0xFFFFFFFFu;
    if (L.beacon_on) {
        const uint64_t slot = cfg.beacon_band_slot, pb = 9ull * cfg.beacon_words_period - 1u, cyc = 9ull * cfg.beacon_words_period;
        next = B ? B + (B - 1 < slot ? 0 : 1 + (B - 1 - slot) / pb) : 0;          // framed position behind the last body symbol (as the encoder counts)
        for (uint64_t q = next; q < L.body_syms_framed; ++q) if (q >= slot && (q - slot) % cyc == 0) e.tail_skip = (uint32_t)(q - next);
    }
    e.tail_off = L.header_syms + next;
    e.tail_len = (uint32_t)(9 * L.out_words - e.tail_off);
}
// A launch of a fused kernel `fn` over n_frames frames (0: the single-frame kernels): the decode planner's repair form for frame 0, bound,
// and the edge.  Three workgroups per CU and a tail within a word, or T3_E_ARG.
int repair_fx_args(RepairFxArgs& ra, uint32_t* grid, void* d_io, const t3_cfg& cfg, const t3_layout& L, const t3_repair_plan& P, const ScrCycle& sc, uint32_t flags,
                   uint32_t* d_verdict, uint32_t n_frames, const void* fn) {
    FusedPlan p; { const int rc = plan_fixed_fused(P.in_bytes, L.header_syms, L, sc, 0, FusedForm::Repair, p); if (rc) return rc == 1 ? T3_E_ARG : rc; }
    memset(&ra, 0, sizeof ra);
    fill_edge(ra.e, cfg, L, d_io, flags, d_verdict);
    if (p.a.lds_bytes > kLdsThreeWgs || ra.e.tail_len > 8u) return T3_E_ARG;
    { const int rc = bind_fused(p, nullptr, nullptr, n_frames, fn); if (rc) return rc; }
    ra.a = p.a; ra.a.in = (const uint8_t*)d_io; *grid = p.grid;
    return T3_OK;
}
// the two kinds (t3_ctx.hpp), kernels by k index; file-local: what other units see is emitted for the device too, which only declares them
#define T3_FOUR_R(kernel) {(const void*)kernel<2>, (const void*)kernel<4>, (const void*)kernel<6>, (const void*)kernel<8>}
const RepairKind kPlain = {4u, T3_FOUR_R(repair_fixed_kernel), T3_FOUR_R(repair_frames_kernel), (const void*)repair_generic_kernel};
const RepairKind kErasures = {6u, T3_FOUR_R(erasure_fixed_kernel), T3_FOUR_R(erasure_frames_kernel), (const void*)erasure_generic_kernel};
#undef T3_FOUR_R
}  // namespace

namespace t3 {
const RepairKind& repair_erasures() { return kErasures; }

// (t3_ctx.hpp: also the erasure decoder's path 0, t3_api_decode_era.cpp)
// The body of a frame whose configuration is known: verdict words zeroed, [0] by hdr_compare_kernel when `hx` is given (hs symbols),
// then ONE launch of the kernel the plan names.  next: the scrambler's next-state table.
int repair_body(void* d_io, const t3_cfg& cfg, const t3_layout& L, const t3_repair_plan& P, const uint8_t next[3], uint32_t flags,
                uint32_t* d_verdict, const HdrExpect* hx, uint32_t hs, hipStream_t s, const RepairKind& kind) {
    Ctx& c = ctx();
    const ScrCycle sc = scrambler_cycle_from_next(next, cfg.seed_s0);
    HIPCHK(hipMemsetAsync(d_verdict, 0, 4 * kind.nw, s));
    if (hx) { hipLaunchKernelGGL(hdr_compare_kernel, dim3(1), dim3(128), 0, s, (const uint8_t*)d_io, *hx, hs, d_verdict); HIPCHK(hipGetLastError()); }
    if (P.path == 1) {
        const void* fn = kind.fixed[k_index(L.band_k[0])];
        RepairFxArgs ra; uint32_t grid;
        { const int rc = repair_fx_args(ra, &grid, d_io, cfg, L, P, sc, flags, d_verdict, 0, fn); if (rc) return rc; }
        void* args[] = {(void*)&ra};
        HIPCHK(hipLaunchKernel(fn, dim3(grid), dim3(512), args, ra.a.lds_bytes, s));
        return T3_OK;
    }
    RepairGenArgs ra; memset(&ra, 0, sizeof ra);
    DecArgs& a = ra.d;
    a.in = (const uint8_t*)d_io; a.tab = c.d_tab; a.fixed = 1; a.hdr_syms = L.header_syms; a.n_sym = L.n_sym;
    uint64_t total = 0;
    for (int b = 0; b < 9; ++b) { a.band_k[b] = L.band_k[b]; a.band_blocks[b] = L.band_blocks[b]; a.band_first[b] = total; a.band_off[b] = L.band_body_off[b]; total += L.band_blocks[b]; }
    a.total_blocks = total;
    a.beacon_on = L.beacon_on; a.period = cfg.beacon_words_period; a.slot = cfg.beacon_band_slot;
    a.cyc24 = sc.cyc24; a.pre0 = sc.pre[0]; a.pre1 = sc.pre[1];
    fill_edge(ra.e, cfg, L, d_io, flags, d_verdict);
    if (ra.e.tail_len > 8u) return T3_E_ARG;
    if (L.beacon_on) {
        ra.bcn_first = cfg.beacon_band_slot; ra.bcn_step = 9ull * cfg.beacon_words_period;
        ra.n_bcn = L.body_syms_framed > ra.bcn_first ? (L.body_syms_framed - ra.bcn_first + ra.bcn_step - 1) / ra.bcn_step : 0;
        ra.bcn_sym = beacon_symbol(cfg.profile, (uint16_t)(cfg.superframe_words % 5), 0);      // what the encoder writes (OLD:1130)
    }
    void* args[] = {(void*)&ra};
    HIPCHK(hipLaunchKernel(kind.generic, dim3(blocks_for(std::max(total, ra.n_bcn), 1u << 16)), dim3(256), args, 0, s));
    return T3_OK;
}
}  // namespace t3

namespace {
// ---- a batch of equal frames ------------------------------------------------------------------------------------------------------------
// n_frames frames of one known configuration.  Where the plan says one launch (path 1, two frames or more), that or T3_E_ARG, never silently
// a loop: ONE memset of every frame's verdict words, [nw f] by ONE hdr_compare_frames_kernel launch when `hx` is given, ONE launch of the
// kind's batch kernel over the tile space of all frames.  Else the single-frame body frame by frame.  hx: the expected header symbols (null:
// no compare, word 0 of every frame stays 0).
int repair_frames_run(void* d_io, uint64_t stride, uint32_t n_frames, const t3_cfg& cfg, const t3_layout& L, const t3_repair_plan& P, const uint8_t next[3],
                      uint32_t flags, uint32_t* d_verdict, const HdrExpect* hx, uint32_t hs, hipStream_t s, const RepairKind& kind) {
    if (P.path != 1 || n_frames < 2) {
        for (uint32_t f = 0; f < n_frames; ++f) {
            const int rc = repair_body((uint8_t*)d_io + (uint64_t)f * stride, cfg, L, P, next, flags, d_verdict + (uint64_t)kind.nw * f, hx, hs, s, kind);
            if (rc) return rc;
        }
        return T3_OK;
    }
    if ((uint64_t)n_frames * P.n_tiles >= (1ull << 31) || hs > 96u) return T3_E_ARG;
    const ScrCycle sc = scrambler_cycle_from_next(next, cfg.seed_s0);
    const void* fn = kind.frames[k_index(L.band_k[0])];
    RepairFramesArgs fa; memset(&fa, 0, sizeof fa); uint32_t grid;
    { const int rc = repair_fx_args(fa.r, &grid, d_io, cfg, L, P, sc, flags, d_verdict, n_frames, fn); if (rc) return rc; }
    fa.stride = stride; fa.n_frames = n_frames; fa.n_total = n_frames * P.n_tiles; fa.div_tiles = to_dev(fastdiv(P.n_tiles));
    HIPCHK(hipMemsetAsync(d_verdict, 0, 4ull * kind.nw * n_frames, s));
    if (hx) {
        hipLaunchKernelGGL(hdr_compare_frames_kernel, dim3(n_frames), dim3(128), 0, s, (const uint8_t*)d_io, stride, *hx, hs, kind.nw, d_verdict);
        HIPCHK(hipGetLastError());
    }
    void* args[] = {(void*)&fa};
    HIPCHK(hipLaunchKernel(fn, dim3(grid), dim3(512), args, fa.r.a.lds_bytes, s));
    return T3_OK;
}

// ---- the entries, plain or with erasures by `kind` ----------------------------------------------------------------------------------
int repair_frame_async(void* d_io, uint64_t n_in, const t3_cfg* cfg, uint64_t n_raw, uint32_t flags, uint32_t* d_verdict, void* stream, const RepairKind& kind) {
    // what can be refused without a device is refused first
    if (!cfg || !d_verdict || (n_in && !d_io) || ((uintptr_t)d_io & 1u) != 0 || (flags & ~T3_REPAIR_WRITE) != 0) return T3_E_ARG;
    t3_repair_plan P; t3_layout L;
    { const int rc = plan_repair(n_raw, *cfg, P, L); if (rc) return rc; }
    if (L.out_words > n_in) return T3_E_HEADER;                                    // truncated stream
    if (!ctx().ready) return T3_E_NODEVICE;
    const KnownFrame k = known_frame(*cfg, n_raw);
    return repair_body(d_io, *cfg, L, P, k.next, flags, d_verdict, &k.hx, k.hs, (hipStream_t)stream, kind);
}

// The header is repaired from its own codewords (header_codewords, t3_frame_batch.hpp), the body by the launch its plan names.
int repair_profile_dev(void* d_io, uint64_t n_in, t3_cfg* seen, uint32_t flags, uint32_t* counts, void* stream, const RepairKind& kind) {
    if (!seen || !counts || (n_in && !d_io) || ((uintptr_t)d_io & 1u) != 0 || (flags & ~T3_REPAIR_WRITE) != 0) return T3_E_ARG;
    if (seen->mode != T3_MODE_FIXED || seen->profile == T3_RAW_MODE) return T3_E_ARG;
    Ctx& c = ctx(); if (!c.ready) return T3_E_NODEVICE;
    memset(counts, 0, kind.nw * sizeof(uint32_t));
    hipStream_t s = (hipStream_t)stream;
    if (n_in < 10) return T3_E_HEADER;
    uint8_t got[90], fix[90], differs = 0;
    { const int rc = fetch_headers(got, d_io, 90, 1, s); if (rc) return rc; }
    FrameHeader h; t3_repair_plan P; t3_layout L;
    { const int rc = accept_header(got, n_in, *seen, h, L, [&](uint64_t n_raw, const t3_cfg& cfg, t3_layout& l) {
          return header_codewords(got, fix, &differs) ? plan_repair(n_raw, cfg, P, l) : T3_E_HEADER; });
      if (rc) return rc == T3_E_ARG ? T3_E_HEADER : rc; }                           // (the plan's: a header that names a framing nobody encodes)
    *seen = h.cfg;                                                                 // the header decoded (OLD:1006-1013)
    void* d_v; { const int rc = scratch(c, Scratch::StreamWork, 64, &d_v, s); if (rc) return rc; }
    { const int rc = repair_body(d_io, h.cfg, L, P, h.next, flags, (uint32_t*)d_v, nullptr, 0, s, kind); if (rc) return rc; }
    if (differs && (flags & T3_REPAIR_WRITE)) HIPCHK(hipMemcpyAsync(d_io, fix, 90, hipMemcpyHostToDevice, s));
    int frc; { const int rc = fetch_verdicts(d_v, kind.nw, 1, nullptr, counts, &frc, s); if (rc) return rc; }
    counts[0] = differs;
    return frc;
}

int repair_profile(void* io, uint64_t n_in, t3_cfg* seen, uint32_t flags, uint32_t* counts, const RepairKind& kind) {
    if (!seen || !counts || (n_in && !io) || (flags & ~T3_REPAIR_WRITE) != 0) return T3_E_ARG;
    if (seen->mode != T3_MODE_FIXED || seen->profile == T3_RAW_MODE) return T3_E_ARG;
    Ctx& c = ctx(); if (!c.ready) return T3_E_NODEVICE;
    std::lock_guard<std::recursive_mutex> hl(c.host_mu);                           // one caller at a time on the shared stream and scratch
    void* di; { const int rc = scratch(c, Scratch::HostIn, n_in * 9 + 64, &di); if (rc) return rc; }
    hipStream_t s = c.stream;
    if (n_in) HIPCHK(hipMemcpyAsync(di, io, n_in * 9, hipMemcpyHostToDevice, s));
    const int rc = repair_profile_dev(di, n_in, seen, flags, counts, s, kind);
    if (rc != T3_OK && rc != T3_E_RS) return rc;
    if ((flags & T3_REPAIR_WRITE) && (counts[0] | counts[3])) {                    // something changed: the one download
        HIPCHK(hipMemcpyAsync(io, di, n_in * 9, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
    }
    return rc;
}

int repair_frames_async(void* d_io, uint64_t n_in, uint64_t stride, uint32_t n_frames, const t3_cfg* cfg, uint64_t n_raw, uint32_t flags,
                        uint32_t* d_verdict, void* stream, const RepairKind& kind) {
    // what can be refused without a device is refused first
    if (!cfg || (flags & ~T3_REPAIR_WRITE) != 0) return T3_E_ARG;
    if (n_frames && (!d_verdict || (n_in && !d_io) || !batch_in_ok(d_io, n_in, stride, n_frames))) return T3_E_ARG;
    t3_repair_frames_plan fp; t3_repair_plan P; t3_layout L;
    { const int rc = plan_repair_frames(n_raw, n_frames, *cfg, fp, P, L); if (rc) return rc; }
    if (n_frames == 0) return T3_OK;
    if (n_frames == 1) return repair_frame_async(d_io, n_in, cfg, n_raw, flags, d_verdict, stream, kind);
    if (L.out_words > n_in) return T3_E_HEADER;                                    // truncated streams
    if (!ctx().ready) return T3_E_NODEVICE;
    const KnownFrame k = known_frame(*cfg, n_raw);
    return repair_frames_run(d_io, stride, n_frames, *cfg, L, P, k.next, flags, d_verdict, &k.hx, k.hs, (hipStream_t)stream, kind);
}

int repair_frames_dev(void* d_io, uint64_t n_in, uint64_t stride, uint32_t n_frames, t3_cfg* seen, uint32_t flags, uint32_t* counts, int* frame_rc,
                      void* stream, const RepairKind& kind) {
    if (!seen || (flags & ~T3_REPAIR_WRITE) != 0 || n_frames > kRepairMaxFrames) return T3_E_ARG;
    if (n_frames && (!counts || !frame_rc || (n_in && !d_io) || !batch_in_ok(d_io, n_in, stride, n_frames))) return T3_E_ARG;
    if (seen->mode != T3_MODE_FIXED || seen->profile == T3_RAW_MODE) return T3_E_ARG;
    if (n_frames == 0) return T3_OK;
    Ctx& c = ctx(); if (!c.ready) return T3_E_NODEVICE;
    const uint32_t nw = kind.nw;
    memset(counts, 0, (uint64_t)nw * n_frames * sizeof(uint32_t));
    for (uint32_t f = 0; f < n_frames; ++f) frame_rc[f] = T3_E_HEADER;
    hipStream_t s = (hipStream_t)stream;
    if (n_in < 10) return T3_E_HEADER;
    std::vector<uint8_t> got(90ull * n_frames), fix(90ull * n_frames), differs(n_frames), go(n_frames);
    { const int rc = fetch_headers(got.data(), d_io, stride, n_frames, s); if (rc) return rc; }
    std::vector<FrameHeader> hd(n_frames); std::vector<t3_repair_plan> P(n_frames); std::vector<t3_layout> L(n_frames);
    if (!parse_headers(got.data(), n_frames, n_in, seen, hd.data(), L.data(), go.data(), [&](uint32_t f, uint64_t n_raw, const t3_cfg& cfg, t3_layout& l) {
            return header_codewords(&got[90ull * f], &fix[90ull * f], &differs[f]) ? plan_repair(n_raw, cfg, P[f], l) : T3_E_HEADER; }))
        return T3_E_HEADER;
    void* d_v; { const int rc = scratch(c, Scratch::StreamWork, 4ull * nw * n_frames + 64, &d_v, s); if (rc) return rc; }
    for (uint32_t f0 = 0, f1 = 0; next_run(go.data(), hd.data(), n_frames, f1, &f0, &f1);) {      // one batched body repair each
        const int rc = repair_frames_run((uint8_t*)d_io + (uint64_t)f0 * stride, stride, f1 - f0, hd[f0].cfg, L[f0], P[f0], hd[f0].next, flags,
                                         (uint32_t*)d_v + (uint64_t)nw * f0, nullptr, 0, s, kind);
        if (rc) return rc;
    }
    if (flags & T3_REPAIR_WRITE)
        for (uint32_t f = 0; f < n_frames; ++f)
            if (go[f] && differs[f]) HIPCHK(hipMemcpyAsync((uint8_t*)d_io + (uint64_t)f * stride, &fix[90ull * f], 90, hipMemcpyHostToDevice, s));
    { const int rc = fetch_verdicts(d_v, nw, n_frames, go.data(), counts, frame_rc, s); if (rc) return rc; }
    for (uint32_t f = 0; f < n_frames; ++f) if (go[f]) counts[nw * f] = differs[f];
    return T3_OK;
}

int repair_frames(void* io, uint64_t n_in, uint64_t stride, uint32_t n_frames, t3_cfg* seen, uint32_t flags, uint32_t* counts, int* frame_rc, const RepairKind& kind) {
    if (!seen || (flags & ~T3_REPAIR_WRITE) != 0 || n_frames > kRepairMaxFrames || n_in > (1ull << 40)) return T3_E_ARG;   // (9 n_in x n_frames fits 64 bits)
    if (n_frames && (!counts || !frame_rc || (n_in && !io) || (n_frames > 1 && stride < 9 * n_in))) return T3_E_ARG;
    if (seen->mode != T3_MODE_FIXED || seen->profile == T3_RAW_MODE) return T3_E_ARG;
    if (n_frames == 0) return T3_OK;
    Ctx& c = ctx(); if (!c.ready) return T3_E_NODEVICE;
    std::lock_guard<std::recursive_mutex> hl(c.host_mu);                           // one caller at a time on the shared stream and scratch
    const FrameStage g = frame_stage(n_in, stride, n_frames);                      // only the frames' bytes travel, up and down
    void* di; { const int rc = scratch(c, Scratch::HostIn, (size_t)(g.dev_stride * n_frames + 64), &di); if (rc) return rc; }
    hipStream_t s = c.stream;
    if (g.bytes) HIPCHK(hipMemcpy2DAsync(di, g.dev_stride, io, g.pitch, g.bytes, n_frames, hipMemcpyHostToDevice, s));
    const int rc = repair_frames_dev(di, n_in, g.dev_stride, n_frames, seen, flags, counts, frame_rc, s, kind);
    if (rc != T3_OK) return rc;
    uint32_t changed = 0;
    for (uint32_t f = 0; f < n_frames; ++f) changed |= counts[kind.nw * f] | counts[kind.nw * f + 3];
    if ((flags & T3_REPAIR_WRITE) && changed) {                                    // something changed: the one download
        HIPCHK(hipMemcpy2DAsync(io, g.pitch, di, g.dev_stride, g.bytes, n_frames, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
    }
    return rc;
}
}  // namespace

extern "C" {

int t3hip_repair_plan(uint64_t n_raw, const t3_cfg* cfg, t3_repair_plan* out) {
    if (!cfg || !out) return T3_E_ARG;
    t3_layout L; return plan_repair(n_raw, *cfg, *out, L);
}
int t3hip_repair_frames_plan(uint64_t n_raw, uint32_t n_frames, const t3_cfg* cfg, t3_repair_frames_plan* out) {
    if (!cfg || !out) return T3_E_ARG;
    t3_repair_plan P; t3_layout L; return plan_repair_frames(n_raw, n_frames, *cfg, *out, P, L);
}

int t3hip_repair_frame_async(void* d_io, uint64_t n_in, const t3_cfg* cfg, uint64_t n_raw, uint32_t flags, uint32_t* d_verdict, void* stream) {
    return repair_frame_async(d_io, n_in, cfg, n_raw, flags, d_verdict, stream, kPlain);
}
int t3hip_repair_profile_dev(void* d_io, uint64_t n_in, t3_cfg* seen, uint32_t flags, uint32_t counts[4], void* stream) {
    return repair_profile_dev(d_io, n_in, seen, flags, counts, stream, kPlain);
}
int t3hip_repair_profile(void* io, uint64_t n_in, t3_cfg* seen, uint32_t flags, uint32_t counts[4]) { return repair_profile(io, n_in, seen, flags, counts, kPlain); }
int t3hip_repair_frames_async(void* d_io, uint64_t n_in, uint64_t stride, uint32_t n_frames, const t3_cfg* cfg, uint64_t n_raw, uint32_t flags, uint32_t* d_verdict, void* stream) {
    return repair_frames_async(d_io, n_in, stride, n_frames, cfg, n_raw, flags, d_verdict, stream, kPlain);
}
int t3hip_repair_frames_dev(void* d_io, uint64_t n_in, uint64_t stride, uint32_t n_frames, t3_cfg* seen, uint32_t flags, uint32_t* counts, int* frame_rc, void* stream) {
    return repair_frames_dev(d_io, n_in, stride, n_frames, seen, flags, counts, frame_rc, stream, kPlain);
}
int t3hip_repair_frames(void* io, uint64_t n_in, uint64_t stride, uint32_t n_frames, t3_cfg* seen, uint32_t flags, uint32_t* counts, int* frame_rc) {
    return repair_frames(io, n_in, stride, n_frames, seen, flags, counts, frame_rc, kPlain);
}
// ... with received bytes above 26 taken as erasures: six words per frame
int t3hip_repair_erasures_frame_async(void* d_io, uint64_t n_in, const t3_cfg* cfg, uint64_t n_raw, uint32_t flags, uint32_t* d_verdict, void* stream) {
    return repair_frame_async(d_io, n_in, cfg, n_raw, flags, d_verdict, stream, kErasures);
}
int t3hip_repair_erasures_profile_dev(void* d_io, uint64_t n_in, t3_cfg* seen, uint32_t flags, uint32_t counts[6], void* stream) {
    return repair_profile_dev(d_io, n_in, seen, flags, counts, stream, kErasures);
}
int t3hip_repair_erasures_profile(void* io, uint64_t n_in, t3_cfg* seen, uint32_t flags, uint32_t counts[6]) { return repair_profile(io, n_in, seen, flags, counts, kErasures); }
int t3hip_repair_erasures_frames_async(void* d_io, uint64_t n_in, uint64_t stride, uint32_t n_frames, const t3_cfg* cfg, uint64_t n_raw, uint32_t flags, uint32_t* d_verdict, void* stream) {
    return repair_frames_async(d_io, n_in, stride, n_frames, cfg, n_raw, flags, d_verdict, stream, kErasures);
}
int t3hip_repair_erasures_frames_dev(void* d_io, uint64_t n_in, uint64_t stride, uint32_t n_frames, t3_cfg* seen, uint32_t flags, uint32_t* counts, int* frame_rc, void* stream) {
    return repair_frames_dev(d_io, n_in, stride, n_frames, seen, flags, counts, frame_rc, stream, kErasures);
}
int t3hip_repair_erasures_frames(void* io, uint64_t n_in, uint64_t stride, uint32_t n_frames, t3_cfg* seen, uint32_t flags, uint32_t* counts, int* frame_rc) {
    return repair_frames(io, n_in, stride, n_frames, seen, flags, counts, frame_rc, kErasures);
}

// ---- block level, bytes above 26 as erasures (FIXED arithmetic only) -------------------------------------------------------------------
int t3hip_rs_decode_block_erasures_host(int k, uint8_t* code26, uint8_t* data_k) {
    if (!valid_k(k) || !code26 || !data_k) return T3_E_ARG;
    uint8_t c[26]; uint32_t mask = 0;
    for (int i = 0; i < 26; ++i) { mask |= (code26[i] > 26u ? 1u : 0u) << i; c[i] = code26[i] % 27u; }
    if (!rs_decode_erasures_host(k, c, mask)) return 0;                            // the block and data_k untouched
    memcpy(code26, c, 26); memcpy(data_k, c, (size_t)k);
    return 1;
}
int t3hip_rs_decode_blocks_erasures_dev(int k, uint8_t* d_code, uint64_t n_blocks, uint8_t* d_data, uint8_t* d_ok, void* stream) {
    if (!valid_k(k) || (n_blocks && (!d_code || !d_data || !d_ok))) return T3_E_ARG;
    Ctx& c = ctx(); if (!c.ready) return T3_E_NODEVICE;
    if (!n_blocks) return T3_OK;
    hipLaunchKernelGGL(rs_erasure_blocks_kernel, dim3((unsigned)((n_blocks + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_code, n_blocks, k, c.d_tab, d_data, d_ok);
    HIPCHK(hipGetLastError()); return T3_OK;
}
int t3hip_rs_decode_blocks_erasures(int k, uint8_t* code26, uint64_t n_blocks, uint8_t* data_k, uint8_t* ok) {
    if (!valid_k(k) || (n_blocks && (!code26 || !data_k || !ok)) || n_blocks > (1ull << 40)) return T3_E_ARG;
    Ctx& c = ctx(); if (!c.ready) return T3_E_NODEVICE;
    if (!n_blocks) return T3_OK;
    std::lock_guard<std::recursive_mutex> lk(c.host_mu);
    void *dc, *dd; int rc = scratch(c, Scratch::HostIn, n_blocks * 26 + 64, &dc); if (rc) return rc;
    rc = scratch(c, Scratch::HostOut, n_blocks * (k + 1) + 64, &dd); if (rc) return rc;
    uint8_t* dok = (uint8_t*)dd + n_blocks * k;
    hipStream_t s = c.stream;
    HIPCHK(hipMemcpyAsync(dc, code26, n_blocks * 26, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dd, data_k, n_blocks * k, hipMemcpyHostToDevice, s));   // data_k of a refused block comes back as it went in
    rc = t3hip_rs_decode_blocks_erasures_dev(k, (uint8_t*)dc, n_blocks, (uint8_t*)dd, dok, s); if (rc) return rc;
    HIPCHK(hipMemcpyAsync(code26, dc, n_blocks * 26, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(data_k, dd, n_blocks * k, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(ok, dok, n_blocks, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s)); return T3_OK;
}

}  // extern "C"
