// t3_api_decode_era.cpp — decode of a FIXED frame with received bytes above 26 taken as erasures, the input read-only (include/t3hip.h,
// "decode with erasures"): the planner's C entry, the asynchronous body decode -- path 1: ONE launch of decode_era_px_kernel
// (t3_decode_era.hip) on the caller's buffer; path 0: a private copy, the erasure repair body on it (repair_body, t3_api_repair.cpp), the
// streaming decoder on the copy -- the synchronous device entry (header parsed on the host) and the host-buffer entry.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <mutex>

#include "../../include/t3hip.h"
#include "t3_ctx.hpp"
#include "t3_dec_plan.hpp"
#include "t3_decode.h"
#include "t3_host.hpp"

using namespace t3;

namespace {
constexpr uint64_t kEraWorkBytes = 128;        // behind the private copy: [0, 24) the repair's six words, [32, 36) the decoder's counter, [64, 80) the synchronous entry's verdict
uint64_t unit_bytes(int fmt) { return fmt == 0 ? 9u : fmt == 1 ? 6u : 3u; }
uint64_t era_scratch_bytes(const t3_decode_erasures_plan& P, uint64_t n_in) { return std::max<uint64_t>(P.scratch_bytes, (9 * n_in + 15u) & ~15ull); }

// what can be refused without a device, in the entries' order: arguments and capacity, then a truncated stream
int era_check(const void* d_in, uint64_t n_in, const void* d_out, uint64_t cap_units, int fmt, const t3_decode_erasures_plan& P, const t3_layout& L) {
    if ((n_in && !d_in) || ((uintptr_t)d_in & 1u) != 0 || n_in > (~0ull) / 9) return T3_E_ARG;
    if (P.out_units && !d_out) return T3_E_ARG;
    if (fmt == 1 && ((uintptr_t)d_out & 1u) != 0) return T3_E_ARG;                  // (t3hip_decode_frame_async: 16-bit components)
    if (P.path == 1 && ((uintptr_t)d_out & 15u) != 0) return T3_E_ARG;              // the fused kernel's stores; never silently path 0
    if (cap_units < P.out_units) return T3_E_CAPACITY;
    if (L.out_words > n_in) return T3_E_HEADER;                                    // truncated stream
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
    { const int rc = repair_body(d_c, cfg, L, rp, next, T3_REPAIR_WRITE, rep6, hx, hs, s, true); if (rc) return rc; }
    uint64_t n_units = 0;
    { const int rc = decode_body_known(d_c, n_in, cfg, n_raw, next, d_out, P.out_units, &n_units, fmt, rep6 + 8, s); if (rc) return rc < 0 ? rc : T3_E_ARG; }
    hipLaunchKernelGGL(era_verdict_kernel, dim3(1), dim3(64), 0, s, (const uint32_t*)rep6, d_verdict);
    HIPCHK(hipGetLastError());
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
    *n_out = P.out_units;                                                          // (what T3_E_CAPACITY asks for)
    { const int rc = era_check(d_in, n_in, d_out, cap_units, fmt, P, L); if (rc) return rc; }
    if (!ctx().ready) return T3_E_NODEVICE;
    HdrExpect hx; memset(&hx, 0, sizeof hx);
    const uint32_t hs = (uint32_t)header_encode(*cfg, n_raw, hx.b);
    const ScrCycle sc = scrambler_cycle(cfg->seed_a, cfg->seed_b, cfg->seed_s0);
    return era_body(d_in, n_in, *cfg, n_raw, L, P, sc.next, d_out, fmt, d_verdict, &hx, hs, (hipStream_t)stream);
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
    HIPCHK(hipMemcpyAsync(got, d_in, 90, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    t3_cfg cfg = *seen; uint64_t n_raw = 0; uint8_t next[3];
    if (header_parse(got, n_in, T3_MODE_FIXED, cfg, &n_raw, next) != T3_OK) return T3_E_HEADER;
    t3_decode_erasures_plan P; t3_layout L;
    { const int rc = plan_decode_erasures(n_raw, cfg, fmt, P, L); if (rc) return rc == T3_E_ARG ? T3_E_HEADER : rc; }   // a header that names a framing nobody encodes
    { const int rc = era_check(d_in, n_in, d_out, cap_units, fmt, P, L); if (rc) { if (rc == T3_E_CAPACITY) *n_out = P.out_units; return rc; } }
    *seen = cfg;                                                                   // the header decoded (OLD:1006-1013)
    const uint64_t cb = P.path == 1 ? 0 : era_scratch_bytes(P, n_in);              // (path 0 asks for the same bytes: the scratch does not move)
    void* d_w; { const int rc = scratch(c, Scratch::StreamErasure, cb + kEraWorkBytes, &d_w, s); if (rc) return rc; }
    uint32_t* const d_v = (uint32_t*)((uint8_t*)d_w + cb + 64);
    { const int rc = era_body(d_in, n_in, cfg, n_raw, L, P, next, d_out, fmt, d_v, nullptr, 0, s); if (rc) return rc; }
    uint32_t v[4];
    HIPCHK(hipMemcpyAsync(v, d_v, 16, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    for (int i = 1; i < 4; ++i) counts[i] = v[i];
    *n_out = P.out_units;
    return v[1] ? T3_E_RS : T3_OK;
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

}  // extern "C"
