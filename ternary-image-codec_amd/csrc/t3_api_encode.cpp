// t3_api_encode.cpp — the encode half of the C-ABI (include/t3hip.h): the encoder's table caches, the K2 dispatch of a frame (planned, then
// launched; the tile itself: t3_enc_plan.cpp), the device and host-buffer encode entry points, batches of equal frames.
// Host logic only; all arithmetic on the data path happens in the kernels (t3_encode.h, t3_kernels.hip).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <mutex>
#include <vector>

#include "../../include/t3hip.h"
#include "t3_ctx.hpp"
#include "t3_dec_plan.hpp"
#include "t3_decode.h"
#include "t3_enc_plan.hpp"
#include "t3_host.hpp"
#include "t3_kernels.h"

using namespace t3;

namespace {

// The encoder's table cache (c.luts; the caller holds c.mu): the tables of `key`, built by build(L, img, afrag) -- the LDS image, the
// single-k launches' A operand, L.k_off -- and uploaded on first use
template <class Build> int cached_lut(Ctx& c, uint32_t key, const LutImage** out, Build build) {
    auto it = c.luts.find(key);
    if (it == c.luts.end()) {
        LutImage L; std::vector<uint32_t> img, afrag; build(L, img, afrag);
        L.bytes = (uint32_t)img.size() * 4u;
        HIPCHK(hipMalloc((void**)&L.d_img, L.bytes ? L.bytes : 16)); HIPCHK(hipMemcpy(L.d_img, img.data(), L.bytes, hipMemcpyHostToDevice));
        if (!afrag.empty()) { HIPCHK(hipMalloc((void**)&L.d_afrag, afrag.size() * 4)); HIPCHK(hipMemcpy(L.d_afrag, afrag.data(), afrag.size() * 4, hipMemcpyHostToDevice)); }
        it = c.luts.emplace(key, L).first;
    }
    *out = &it->second;
    return T3_OK;
}
using Words = std::vector<uint32_t>;
// tables of the LUT kernel: the LUT of every k in use, one behind the other (k_off = its offset)
int get_lut(Ctx& c, uint32_t kmask, int mode, const LutImage** out) {
    return cached_lut(c, kmask | (uint32_t)mode << 8, out, [&](LutImage& L, Words& all, Words&) {
        for (int i = 0; i < 4; ++i) if (kmask >> i & 1) {
            Words img; build_encode_lut(kOfIndex[i], mode, img);
            L.k_off[i] = (uint32_t)all.size() * 4u;
            all.insert(all.end(), img.begin(), img.end());
        }
    });
}
// tables of the matrix-core encoder for one k (single-k launches)
int get_mfma_lut(Ctx& c, int k, int mode, const LutImage** out) {
    return cached_lut(c, 1u << k_index(k) | (uint32_t)mode << 8 | 1u << 16, out, [&](LutImage&, Words& img, Words& afrag) { build_mfma_encode(k, mode, afrag, img); });
}
// tables of the UEP matrix-core kernel: the k-independent T/M image, then the A operand of every k in use (k_off = its offset)
int get_mfma_group_lut(Ctx& c, uint32_t kmask, int mode, const LutImage** out) {
    return cached_lut(c, kmask | (uint32_t)mode << 8 | 2u << 16, out, [&](LutImage& L, Words& all, Words&) {
        for (int i = 0; i < 4; ++i) if (kmask >> i & 1) {
            Words afrag, img; build_mfma_encode(kOfIndex[i], mode, afrag, img);
            if (all.empty()) all = img;                                   // T and M tables do not depend on k
            L.k_off[i] = (uint32_t)all.size() * 4u;
            all.insert(all.end(), afrag.begin(), afrag.end());
        }
    });
}

struct EncPlan { EncLaunch l[2]; uint32_t n = 0; bool beacon_pass = false; BeaconArgs b; };   // a frame's launches, then the beacon pass

// The kernel of a launch (t3_encode_px.hip, t3_encode_words.hip and t3_encode_rgb.hip instantiate every one).  il: the 2-D flow of encode_body -- 0 1-D, 1 the tile's rows staged
// whole (raw words' only 2-D flow), 2 runs; r = 26 - k of a single-k launch; bcn: the beacon fused into the stores (not the LUT kernel's).
const void* enc_kernel(int fe, uint32_t il, EncKind kind, uint32_t r, bool bcn) {
#define T3_PICKB(FE, IL, B) (kind == EncKind::Lut ? (const void*)encode_kernel_mixed<FE, IL> : kind == EncKind::Uep ? (const void*)encode_kernel_uep<FE, IL, B> \
                             : r == 2 ? (const void*)encode_kernel_k<FE, IL, 2, B> : r == 4 ? (const void*)encode_kernel_k<FE, IL, 4, B>                  \
                             : r == 6 ? (const void*)encode_kernel_k<FE, IL, 6, B> : (const void*)encode_kernel_k<FE, IL, 8, B>)
#define T3_PICK(FE, IL) (bcn ? T3_PICKB(FE, IL, true) : T3_PICKB(FE, IL, false))
    if (fe == FE_WORDS) return il ? T3_PICK(FE_WORDS, 1) : T3_PICK(FE_WORDS, 0);
    if (fe == FE_RGB) return il == 2 ? T3_PICK(FE_RGB, 2) : il ? T3_PICK(FE_RGB, 1) : T3_PICK(FE_RGB, 0);
    return il == 2 ? T3_PICK(FE_PIXELS, 2) : il ? T3_PICK(FE_PIXELS, 1) : T3_PICK(FE_PIXELS, 0);
#undef T3_PICK
#undef T3_PICKB
}

#ifdef T3_STAMPS
// Stamp build (-DT3_STAMPS): the kernels' per-workgroup stamps of one launch of `grid` workgroups, summarised on stderr
int stamps_report(const EncLaunch& e, const uint64_t* d_dbg, uint32_t grid, hipStream_t s) {
    std::vector<uint64_t> h16(16 * grid), h(8 * grid);
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipMemcpy(h16.data(), d_dbg, h16.size() * 8, hipMemcpyDeviceToHost));
    for (uint32_t w = 0; w < grid; ++w) for (int i = 0; i < 8; ++i) h[8 * w + i] = h16[16 * w + i];
    { std::map<uint32_t, std::vector<uint32_t>> per_cu; double xl[8] = {0}; int xn[8] = {0};
      for (uint32_t w = 0; w < grid; ++w) { const uint32_t hw = (uint32_t)h16[16 * w + 8], xcc = (uint32_t)h16[16 * w + 9] & 15u;
          per_cu[xcc << 16 | (hw >> 8 & 0xFFu)].push_back((uint32_t)h[8 * w + 5]); xl[xcc & 7] += (double)h[8 * w + 5] * 0.01; ++xn[xcc & 7]; }
      int hist[8] = {0}; for (auto& kv : per_cu) ++hist[std::min<size_t>(kv.second.size(), 7)];
      fprintf(stderr, "[t3 stamps]   CUs seen=%zu  CUs holding n WGs: 1:%d 2:%d 3:%d 4:%d 5:%d 6+:%d\n", per_cu.size(), hist[1], hist[2], hist[3], hist[4], hist[5], hist[6] + hist[7]);
      fprintf(stderr, "[t3 stamps]   mean WG lifetime (us) per XCC:"); for (int x = 0; x < 8; ++x) fprintf(stderr, " %d:%.1f(n=%d)", x, xn[x] ? xl[x] / xn[x] : 0.0, xn[x]); fprintf(stderr, "\n");
      double ln[8] = {0}; int cn[8] = {0}; for (auto& kv : per_cu) { const size_t n = std::min<size_t>(kv.second.size(), 7); for (uint32_t v : kv.second) { ln[n] += v * 0.01; ++cn[n]; } }
      fprintf(stderr, "[t3 stamps]   mean WG lifetime (us) by WGs on its CU:"); for (int n = 1; n < 8; ++n) if (cn[n]) fprintf(stderr, " %d:%.1f", n, ln[n] / cn[n]); fprintf(stderr, "\n");
      fprintf(stderr, "[t3 stamps]   hw_id samples: %08x %08x %08x %08x\n", (unsigned)h16[8], (unsigned)h16[16 + 8], (unsigned)h16[32 + 8], (unsigned)h16[16 * 100 + 8]); }
    double acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (uint32_t w = 0; w < grid; ++w) for (int i = 0; i < 8; ++i) acc[i] += (double)h[8 * w + i];
    fprintf(stderr, "[t3 stamps] grid=%u tiles=%u  mean cycles/WG: stage=%.0f p1=%.0f p2=%.0f p3=%.0f total=%.0f  clock=%.3f GHz\n", grid, e.a.n_tiles,
            acc[0] / grid, acc[1] / grid, acc[2] / grid, acc[3] / grid, acc[4] / grid, acc[4] / acc[5] * 0.1);
    { uint64_t s0 = ~0ull, s1 = 0, e0 = ~0ull, e1 = 0; for (uint32_t w = 0; w < grid; ++w) { const uint64_t st = h[8 * w + 3], en = st + h[8 * w + 5]; s0 = std::min(s0, st); s1 = std::max(s1, st); e0 = std::min(e0, en); e1 = std::max(e1, en); }
      int late = 0; for (uint32_t w = 0; w < grid; ++w) if (h[8 * w + 3] - s0 > 1000) ++late;
      fprintf(stderr, "[t3 stamps]   timeline (us from first start): last start=%.2f first end=%.2f last end=%.2f  WGs starting >10us late=%d\n", (s1 - s0) * 0.01, (e0 - s0) * 0.01, (e1 - s0) * 0.01, late);
      fprintf(stderr, "[t3 stamps]   lds_bytes=%u block=%u\n", e.a.lds_bytes, e.block); }
    fprintf(stderr, "[t3 stamps]   p1 split (wave 0): prefetch issue=%.0f convert=%.0f barrier wait=%.0f\n", acc[6] / grid, acc[7] / grid, acc[1] / grid);
    { double il = 0; for (uint32_t w = 0; w < grid; ++w) il += (double)h16[16 * w + 10]; fprintf(stderr, "[t3 stamps]   2-D permutation pass (in p2): %.0f\n", il / grid); }
    { double pr = 0; for (uint32_t w = 0; w < grid; ++w) pr += (double)h16[16 * w + 11]; fprintf(stderr, "[t3 stamps]   prologue (kernel entry -> first tile's input landed, wave 0): mean %.0f cycles/WG\n", pr / grid); }
    return T3_OK;
}
#endif

// One K2 launch on s (the caller holds c.mu): the resident grid for its tiles, the stream's tile tickets, the kernel
int launch_enc(Ctx& c, EncLaunch& e, hipStream_t s) {
    uint32_t grid; { const int rc = resident_grid(c, e.fn, (int)e.block, e.a.lds_bytes, e.a.n_tiles, true, &grid); if (rc) return rc; }
#ifdef T3_STAMPS
    static uint64_t* d_dbg = nullptr; static int calls = 0;
    if (!d_dbg) HIPCHK(hipMalloc((void**)&d_dbg, 16 * 8 * 4096));
    HIPCHK(hipMemsetAsync(d_dbg, 0, 16 * 8 * 4096, s));
    e.a.dbg = d_dbg;
#endif
    tile_tickets_held(c, s, 0, grid, &e.a.tile_ctr, &e.a.n_classes);
    void* args[] = {(void*)&e.a};
    HIPCHK(hipLaunchKernel(e.fn, dim3(grid), dim3(e.block), args, e.a.lds_bytes, s));
#ifdef T3_STAMPS
    if (++calls == 8) return stamps_report(e, d_dbg, grid, s);       // one report, after warm-up
#endif
    return T3_OK;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// chroma quantiser of the fused RGB front end: C -> clamp(lround((C - 128) * (40.0 / 128.0)), -40, 40) + 40 (io_image.hpp:73-76), the
// reference's own double expression tabulated on the host
int rgb_quant_table(Ctx& c, const uint8_t** out) {                   // caller holds c.mu
    uint8_t*& d_qt = c.rgb.chroma_q;
    if (!d_qt) {
        uint8_t t[256];
        for (int C = 0; C < 256; ++C) { long v = lround((C - 128) * (40.0 / 128.0)); v = v < -40 ? -40 : (v > 40 ? 40 : v); t[C] = (uint8_t)(v + 40); }
        HIPCHK(hipMalloc((void**)&d_qt, sizeof t)); HIPCHK(hipMemcpy(d_qt, t, sizeof t, hipMemcpyHostToDevice));
    }
    *out = d_qt; return T3_OK;
}

// The K2 dispatch of a frame, planned (the caller holds c.mu): builds every table its launches use, picks each launch's kernel and
// fills its arguments but for what depends on the stream; launches nothing.
int plan_encode(Ctx& c, int fe, const void* d_in, uint64_t n_units, const t3_cfg& cfg, const t3_layout& L, void* d_out, EncPlan& p) {
    uint8_t hdr[96]; memset(hdr, 0, sizeof hdr);
    const uint32_t hs = (uint32_t)header_encode(cfg, L.n_raw_words, hdr);
    const uint32_t pad = (uint32_t)(9 * L.out_words - L.out_syms);
    // group bands into launches: all together when the lcm of their k's keeps the LUT kernel's tile small, else one launch per k -- and
    // with three or four different k (the lcm of all of them makes a tile no LDS holds, the lcm of two does) by pairs of k: each launch
    // runs phase 1 over the whole frame and encodes its bands
    uint32_t kmask = 0; for (int b = 0; b < 9; ++b) kmask |= 1u << k_index(L.band_k[b]);
    const bool one_k = (kmask & (kmask - 1)) == 0;                       // one k for all nine bands: matrix-core kernels
    uint32_t groups[2] = {0x1FFu, 0u}; p.n = 1;
    if (!one_k) {
        const LutImage* lut; const int rc = get_lut(c, kmask, cfg.mode, &lut); if (rc) return rc;
        EncLaunch probe;
        if (!plan_enc_group(L, cfg, 0x1FF, fe, lut->bytes, lut->k_off, EncKind::Lut, probe)) {
            uint32_t per_k[4] = {0, 0, 0, 0}, n = 0;
            for (int i = 0; i < 4; ++i) if (kmask >> i & 1) { for (int b = 0; b < 9; ++b) if (k_index(L.band_k[b]) == i) per_k[n] |= 1u << b; ++n; }
            groups[0] = n == 2 ? per_k[0] : per_k[0] | per_k[1]; groups[1] = n == 2 ? per_k[1] : per_k[2] | per_k[3]; p.n = 2;
        }
    }
    // A beacon (OLD:1118-1141) rides in the store addressing of the matrix-core kernels when one launch covers the frame and a 16-byte
    // run can hold one beacon at most (period >= 2); otherwise the body goes to scratch and beacon_kernel frames it.
    const bool bcn_cand = L.beacon_on && cfg.beacon_band_slot < 9 && cfg.beacon_words_period >= 2 && cfg.beacon_words_period < (1u << 27) && !getenv("T3HIP_BEACON_PASS") && p.n == 1;
    const uint8_t bcn_sym = beacon_symbol(cfg.profile, (uint16_t)(cfg.superframe_words % 5), 0);     // OLD:1130
    for (uint32_t g = 0; g < p.n; ++g) {
        const uint32_t m = groups[g];
        uint32_t km = 0; for (int b = 0; b < 9; ++b) if (m >> b & 1) km |= 1u << k_index(L.band_k[b]);
        EncLaunch& e = p.l[g]; const LutImage* lut;
        // the matrix cores when the tile fits eight waves: one k -- 64 or 32 blocks per band and tile; several k in the frame -- the UEP
        // kernel (bands grouped by k; any band subset; always 512 threads); else the LUT kernel
        int rc = one_k ? get_mfma_lut(c, L.band_k[0], cfg.mode, &lut) : get_mfma_group_lut(c, km, cfg.mode, &lut); if (rc) return rc;
        if (!plan_enc_group(L, cfg, m, fe, lut->bytes, lut->k_off, one_k ? EncKind::MfmaK : EncKind::Uep, e) || e.block > 512) {
            rc = get_lut(c, km, cfg.mode, &lut); if (rc) return rc;
            if (!plan_enc_group(L, cfg, m, fe, lut->bytes, lut->k_off, EncKind::Lut, e)) return T3_E_ARG;
        }
        const bool bcn_fused = bcn_cand && e.kind != EncKind::Lut;
        p.beacon_pass = L.beacon_on && !bcn_fused;
        EncArgs& a = e.a;
        a.afrag = e.kind == EncKind::MfmaK ? lut->d_afrag : nullptr; a.lut_img = lut->d_img;
        a.in = (const uint8_t*)d_in; a.n_units = n_units; a.n_units_pad = fe_px(fe) ? 2 * L.n_raw_words : n_units;
        if (fe == FE_RGB) { rc = rgb_quant_table(c, &a.qt); if (rc) return rc; }
        // the body behind the header, or (launch_encode) the beacon pass's scratch; header and pad: the first launch's tile 0, or the pass
        a.body_out = p.beacon_pass ? nullptr : (uint8_t*)d_out + hs; a.frame_out = g == 0 && !p.beacon_pass ? (uint8_t*)d_out : nullptr;
        a.hdr_syms = hs; a.pad_bytes = pad; a.out_syms = L.out_syms; memcpy(a.hdr, hdr, sizeof hdr);
        if (bcn_fused) {
            const uint64_t cyc = 9ull * cfg.beacon_words_period, pb = cyc - 1, B = L.body_syms, slot = cfg.beacon_band_slot;
            a.bcn_slot = (uint32_t)slot; a.bcn_pb = (uint32_t)pb; a.bcn_div = to_dev(fastdiv((uint32_t)pb)); a.bcn_sym = bcn_sym;
            // framed bytes after the last body byte (the rest of the last word): zeros, or a beacon whose slot comes after it
            const uint64_t next = B ? B + (B - 1 < slot ? 0 : 1 + (B - 1 - slot) / pb) : 0;
            a.bcn_tail_off = hs + next; a.bcn_tail_len = (uint32_t)(L.body_syms_framed - next); a.bcn_tail_vals = 0;
            if (a.bcn_tail_len > 8) return T3_E_ARG;                                   // (cannot happen: less than one word)
            for (uint64_t q = next; q < L.body_syms_framed; ++q) if (q >= slot && (q - slot) % cyc == 0) a.bcn_tail_vals |= (uint64_t)bcn_sym << (8 * (q - next));
        }
        e.fn = enc_kernel(fe, !a.il_on ? 0u : a.il_async == 2u ? 2u : 1u, e.kind, 26u - (uint32_t)L.band_k[0], bcn_fused);
    }
    if (p.beacon_pass) {
        BeaconArgs& b = p.b; memset(&b, 0, sizeof b);
        b.frame_out = (uint8_t*)d_out; b.body_syms = L.body_syms; b.framed_syms = L.body_syms_framed;
        b.period = cfg.beacon_words_period; b.slot = cfg.beacon_band_slot; b.sym = bcn_sym;
        b.hdr_syms = hs; b.pad_bytes = pad; memcpy(b.hdr, hdr, sizeof hdr);
    }
    return T3_OK;
}

// Runs a plan on s (the caller holds c.mu).  The beacon pass's body scratch is taken first: once a kernel is enqueued, only the launch
// steps remain.
int launch_encode(Ctx& c, EncPlan& p, hipStream_t s) {
    if (p.beacon_pass) {
        void* body; const int rc = scratch_held(c, Scratch::StreamBody, p.b.body_syms + 64, &body, s); if (rc) return rc;
        p.b.body = (const uint8_t*)body;
        for (uint32_t i = 0; i < p.n; ++i) p.l[i].a.body_out = (uint8_t*)body;
    }
    for (uint32_t i = 0; i < p.n; ++i) { const int rc = launch_enc(c, p.l[i], s); if (rc) return rc; }
    if (p.beacon_pass) {
        hipLaunchKernelGGL(beacon_kernel, dim3(blocks_for((p.b.hdr_syms + p.b.framed_syms + 15) / 16, 65536)), dim3(256), 0, s, p.b);   // one lane per 16-byte granule
        HIPCHK(hipGetLastError());
    }
    return T3_OK;
}

// pixels|raw words (device) -> coded stream (device)
int encode_dev(int fe, const void* d_in, uint64_t n_units, const t3_cfg* cfg, void* d_out, uint64_t cap_words, uint64_t* n_out, hipStream_t s) {
    Ctx& c = ctx(); if (!c.ready) return T3_E_NODEVICE;
    if (fe == FE_RGB && cfg && n_out && d_in && !aligned16(d_in)) return 1;      // the bridge kernel takes any alignment
    const bool raw_mode = cfg && cfg->profile == T3_RAW_MODE;                       // RAW: a copy or the pack kernel, any alignment
    if (!cfg || !n_out || (n_units && !d_in) || (!raw_mode && (!aligned16(d_in) || !aligned16(d_out)))) return T3_E_ARG;
    const uint64_t n_raw = fe_px(fe) ? (n_units + 1) / 2 : n_units;
    t3_layout L; int rc = plan(n_raw, *cfg, L); if (rc != T3_OK) return rc;
    *n_out = L.out_words;
    // the fused RGB front end rides the pipelined flow only: RAW mode and 2-D rows wider than 512 go through the bridge kernel (1 = not taken)
    if (fe == FE_RGB && cfg->profile == T3_RAW_MODE) return 1;
    if (L.out_words > cap_words) return T3_E_CAPACITY;
    if (L.out_words && !d_out) return T3_E_ARG;
    if (cfg->profile == T3_RAW_MODE) {                                   // OLD:1046-1050: out = in
        if (fe == FE_WORDS) { if (n_raw) HIPCHK(hipMemcpyAsync(d_out, d_in, n_raw * 9, hipMemcpyDeviceToDevice, s)); }
        else if (n_raw) { hipLaunchKernelGGL(pack_pixels_kernel, dim3((unsigned)(((n_raw + 3) / 4 + 255) / 256)), dim3(256), 0, s, (const uint16_t*)d_in, n_units, (uint8_t*)d_out, n_raw); HIPCHK(hipGetLastError()); }
        return T3_OK;
    }
    std::lock_guard<std::mutex> lk(c.mu);
    EncPlan p; rc = plan_encode(c, fe, d_in, n_units, *cfg, L, d_out, p); if (rc) return rc;
    return launch_encode(c, p, s);
}

// ------------------------------------------------------------------------------------------------
// Batches of equal frames (t3hip.h): one K2 launch over the tile space of all frames where the single-k matrix-core kernel serves a frame
// (pixel / RGB input, 1-D, no beacon), else a loop of the single-frame entries
// ------------------------------------------------------------------------------------------------
int fe_of_fmt(int fmt) { return fmt == 0 ? FE_WORDS : fmt == 1 ? FE_PIXELS : FE_RGB; }
const void* enc_frames_kernel(int fe, uint32_t r) {      // t3_encode_frames.hip instantiates every one
#define T3_PICKF(FE) (r == 2 ? (const void*)enc_frames_k<FE, 2> : r == 4 ? (const void*)enc_frames_k<FE, 4> : r == 6 ? (const void*)enc_frames_k<FE, 6> : (const void*)enc_frames_k<FE, 8>)
    return fe == FE_RGB ? T3_PICKF(FE_RGB) : T3_PICKF(FE_PIXELS);
#undef T3_PICKF
}
int encode_frames_dev(const void* d_in, uint64_t n_units, int fmt, uint64_t in_stride, uint32_t n_frames, const t3_cfg* cfg, void* d_out, uint64_t out_stride,
                      uint64_t* n_out, hipStream_t s) {
    // what can be refused without a device is refused first: a null base never reaches a launch (0 is 16-byte aligned)
    if (!cfg || !n_out) return T3_E_ARG;
    t3_frames_plan fp; t3_layout L;
    int rc = plan_frames(0, n_units, n_frames, *cfg, fmt, fp, L); if (rc) return rc;
    *n_out = L.out_words;
    if (n_frames && ((n_units && !d_in) || (L.out_words && !d_out))) return T3_E_ARG;        // as the single-frame entries (encode_dev)
    if (n_frames > 1 && !frames_strides_ok(fp, d_in, in_stride, d_out, out_stride)) return T3_E_ARG;
    Ctx& c = ctx(); if (!c.ready) return T3_E_NODEVICE;
    if (n_frames == 0) return T3_OK;
    const int fe = fe_of_fmt(fmt);
    if (fp.one_launch) {
        std::lock_guard<std::mutex> lk(c.mu);
        EncPlan p; rc = plan_encode(c, fe, d_in, n_units, *cfg, L, d_out, p); if (rc) return rc;
        const EncLaunch& e = p.l[0];
        // The frame's plan must be what plan_frames told the caller (one launch of the single-k kernel, 1-D, header and pad from the kernel,
        // that tile): a batch the plan calls one launch runs as one launch or not at all, never silently as the loop below.
        if (!(p.n == 1 && e.kind == EncKind::MfmaK && !p.beacon_pass && !e.a.il_on && !e.a.bcn_pb && e.a.n_tiles == fp.tiles_per_frame && e.block <= 512u)) return T3_E_ARG;
        EncFramesArgs fa; memset(&fa, 0, sizeof fa);
        fa.a = e.a; fa.in_stride = in_stride; fa.out_stride = out_stride; fa.n_frames = n_frames;
        fa.n_total = n_frames * fp.tiles_per_frame; fa.div_tiles = to_dev(fastdiv(fp.tiles_per_frame));
        const void* fn = enc_frames_kernel(fe, 26u - (uint32_t)L.band_k[0]);
        uint32_t grid; rc = resident_grid(c, fn, (int)e.block, fa.a.lds_bytes, fa.n_total, true, &grid); if (rc) return rc;
        tile_tickets_held(c, s, 0, grid, &fa.a.tile_ctr, &fa.a.n_classes);
        void* args[] = {(void*)&fa};
        HIPCHK(hipLaunchKernel(fn, dim3(grid), dim3(e.block), args, fa.a.lds_bytes, s));
        return T3_OK;
    }
    for (uint32_t f = 0; f < n_frames; ++f) {
        const uint8_t* in = (const uint8_t*)d_in + (uint64_t)f * in_stride; uint8_t* out = (uint8_t*)d_out + (uint64_t)f * out_stride; uint64_t n = 0;
        rc = fmt == 0 ? t3hip_encode_profile_dev(in, n_units, cfg, out, L.out_words, &n, s) : fmt == 1 ? t3hip_encode_frame_dev(in, n_units, cfg, out, L.out_words, &n, s)
                      : t3hip_encode_rgb_dev(in, n_units, cfg, out, L.out_words, &n, s);
        if (rc) return rc;
    }
    return T3_OK;
}

}  // namespace

// shared with the other host translation units (t3_ctx.hpp)
namespace t3 {
int plan_frames(int decode, uint64_t n_units, uint32_t n_frames, const t3_cfg& cfg, int fmt, t3_frames_plan& out, t3_layout& L) {
    memset(&out, 0, sizeof out);
    if (fmt < 0 || fmt > 2 || n_frames > 65535u) return T3_E_ARG;
    const uint64_t n_raw = fmt == 0 ? n_units : (n_units + 1) / 2, UB = fmt == 0 ? 9u : fmt == 1 ? 6u : 3u;
    { const int rc = plan(n_raw, cfg, L); if (rc) return rc; }
    out.n_frames = n_frames;
    const uint64_t coded = 9 * L.out_words, units = (decode ? (fmt == 0 ? n_raw : 2 * n_raw) : n_units) * UB;   // a decode emits whole words: the pad pixel too
    out.in_bytes = decode ? coded : units; out.out_bytes = decode ? units : coded;
    out.in_stride_min = (out.in_bytes + 15u) & ~15ull; out.out_stride_min = (out.out_bytes + 15u) & ~15ull;
    // one launch: where the fused single-k kernels serve a frame (plan_encode's matrix-core kernel without beacon; plan_fixed_fused's pixel kernel)
    if (n_frames < 2 || n_raw == 0 || fmt == 0 || cfg.profile == T3_RAW_MODE || !single_k(L) || L.interleave2d || L.beacon_on) return T3_OK;
    uint32_t tiles = 0;
    if (decode) {
        if (cfg.mode != T3_MODE_FIXED || coded >= (1ull << 32) || getenv("T3HIP_GENERIC_DECODE") != nullptr) return T3_OK;
        tiles = fused_tiles(L, FusedForm::Pixels);
    } else {
        const uint32_t no_off[4] = {0, 0, 0, 0}; EncLaunch e;                   // the tile depends on the tables' size alone: no device
        if (!plan_enc_group(L, cfg, 0x1FF, fe_of_fmt(fmt), (uint32_t)kMfmaLdsBytes, no_off, EncKind::MfmaK, e) || e.block > 512u) return T3_OK;
        tiles = e.a.n_tiles;
    }
    if (tiles == 0) return T3_OK;
    if ((uint64_t)n_frames * tiles >= (1ull << 31)) return T3_E_ARG;
    out.tiles_per_frame = tiles; out.one_launch = 1;
    return T3_OK;
}
int encode_rgb_fused(const void* d_rgb, uint64_t n_px, const t3_cfg* cfg, void* d_out, uint64_t cap, uint64_t* n_out, hipStream_t s) { return encode_dev(FE_RGB, d_rgb, n_px, cfg, d_out, cap, n_out, s); }
}  // namespace t3

extern "C" {

// ---- device-resident entry points -----------------------------------------------------------------------
int t3hip_pack_pixels_dev(const void* d_px, uint64_t n_px, void* d_words, void* stream) {
    if (!ctx().ready) return T3_E_NODEVICE;
    const uint64_t nw = (n_px + 1) / 2; if (!nw) return T3_OK;
    if (!d_px || !d_words) return T3_E_ARG;
    hipLaunchKernelGGL(pack_pixels_kernel, dim3((unsigned)(((nw + 3) / 4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const uint16_t*)d_px, n_px, (uint8_t*)d_words, nw);
    HIPCHK(hipGetLastError()); return T3_OK;
}
int t3hip_unpack_words_dev(const void* d_words, uint64_t n_words, void* d_px, void* stream) {
    if (!ctx().ready) return T3_E_NODEVICE;
    if (!n_words) return T3_OK;
    if (!d_px || !d_words) return T3_E_ARG;
    hipLaunchKernelGGL(unpack_words_kernel, dim3((unsigned)(((n_words + 3) / 4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)d_words, n_words, (uint16_t*)d_px);
    HIPCHK(hipGetLastError()); return T3_OK;
}
int t3hip_encode_profile_dev(const void* d_raw, uint64_t n_raw, const t3_cfg* cfg, void* d_out, uint64_t cap, uint64_t* n_out, void* stream) {
    return encode_dev(FE_WORDS, d_raw, n_raw, cfg, d_out, cap, n_out, (hipStream_t)stream);
}
int t3hip_encode_frame_dev(const void* d_px, uint64_t n_px, const t3_cfg* cfg, void* d_out, uint64_t cap, uint64_t* n_out, void* stream) {
    return encode_dev(FE_PIXELS, d_px, n_px, cfg, d_out, cap, n_out, (hipStream_t)stream);
}
int t3hip_rs_encode_blocks_dev(int k, int mode, const uint8_t* d_data, uint64_t n_blocks, uint8_t* d_code, void* stream) {
    Ctx& c = ctx(); if (!c.ready) return T3_E_NODEVICE;
    if (!valid_k(k) || mode < 0 || mode > 1) return T3_E_ARG;
    if (!n_blocks) return T3_OK;
    hipLaunchKernelGGL(rs_encode_blocks_kernel, dim3((unsigned)((n_blocks + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_data, n_blocks, k, c.d_P[k_index(k)][mode], c.d_tab, d_code);
    HIPCHK(hipGetLastError()); return T3_OK;
}

// ---- host-buffer entry points ---------------------------------------------------------------------------
int t3hip_pack_pixels(const void* px, uint64_t n_px, void* words) {
    Ctx& c = ctx(); if (!c.ready) return T3_E_NODEVICE;
    const uint64_t nw = (n_px + 1) / 2; if (!nw) return T3_OK;
    if (!px || !words) return T3_E_ARG;
    std::lock_guard<std::recursive_mutex> hl(c.host_mu);
    void *di, *dout; int rc = host_stage(c, px, n_px * 6, &di, nw * 9, &dout); if (rc) return rc;
    rc = t3hip_pack_pixels_dev(di, n_px, dout, c.stream); if (rc) return rc;
    return host_fetch(c, words, dout, nw * 9);
}
int t3hip_unpack_words(const void* words, uint64_t n_words, void* px) {
    Ctx& c = ctx(); if (!c.ready) return T3_E_NODEVICE;
    if (!n_words) return T3_OK;
    if (!px || !words) return T3_E_ARG;
    std::lock_guard<std::recursive_mutex> hl(c.host_mu);
    void *di, *dout; int rc = host_stage(c, words, n_words * 9, &di, n_words * 12, &dout); if (rc) return rc;
    rc = t3hip_unpack_words_dev(di, n_words, dout, c.stream); if (rc) return rc;
    return host_fetch(c, px, dout, n_words * 12);
}
// Pipelined host entry (round 3): the frame crosses PCIe once in each direction, and the two directions overlap (run_chunks).  Tiles are
// independent, and a range of whole tiles that starts on a pixel-triple / word-triple boundary at a 16-byte aligned input offset
// is a frame of its own to the kernel -- same kernel, shifted pointers and band offsets, no tile-range logic in the hot loop.  Chunk c goes
// up and through the kernel while the nine band runs of chunk c - 1 come down (measured on the box, profiles/exp/pcie_probe.cpp: 3.5 ms up
// + 3.3 ms down one after the other, 4.0-4.2 ms both at once).  One k on all bands, 1-D, no beacon, and the frame's plan one launch of the
// single-k matrix-core kernel, which every chunk runs shifted; anything else: the serial path (1).
static int encode_host_pipelined(Ctx& c, int fe, const void* in, uint64_t n_units, const t3_cfg* cfg, void* out, const t3_layout& L, void* di, void* dout) {
    if (fe == FE_RGB || L.interleave2d || L.beacon_on || cfg->profile == T3_RAW_MODE || getenv("T3HIP_SERIAL_HOST") != nullptr || !single_k(L)) return 1;
    EncPlan p;
    { std::lock_guard<std::mutex> lk(c.mu); const int rc = plan_encode(c, fe, di, n_units, *cfg, L, dout, p); if (rc) return rc; }
    if (p.n != 1 || p.l[0].kind != EncKind::MfmaK || p.beacon_pass) return 1;
    const EncLaunch& e0 = p.l[0];
    const uint32_t hs = e0.a.hdr_syms, TS = 9u * e0.a.Lq, unit_syms = fe == FE_PIXELS ? 104u : 416u;     // chunk starts: whole triples at 16-byte aligned input offsets
    const uint32_t G = unit_syms / (uint32_t)gcd64(TS, unit_syms);                     // tiles per alignment unit
    const uint32_t n_tiles = e0.a.n_tiles;
    // chunks: fill / drain of the pipeline against per-copy overheads.  The nine band runs of a chunk go down as ONE strided copy when the
    // bands are equally long and everything is 4-byte aligned (COMPAT: 52 header symbols; measured 4.70 ms per 8K frame with 12 chunks);
    // a strided copy at 2-byte alignment (FIXED: 90 header symbols) falls off a cliff (13 ms), so there: nine plain copies, 6 chunks (5.1 ms)
    const bool allow_strided = hs % 4u == 0 && getenv("T3HIP_NO_2D_COPY") == nullptr;
    const uint32_t per = (n_tiles / host_chunks(allow_strided && equal_band_runs(L) ? 12u : 6u) + G - 1u) / G * G;
    if (per == 0 || n_tiles < 4u * G) return 1;                                      // small frames: the serial path
    const uint32_t n_chunks = (n_tiles + per - 1u) / per;
    const uint32_t UB = fe == FE_PIXELS ? 6u : 9u, nb = e0.a.nb_uniform;
    const uint64_t in_bytes = n_units * UB;
    uint8_t* const ho = (uint8_t*)out; const uint8_t* const dob = (const uint8_t*)dout;
    uint64_t up_done = 0;
    return run_chunks(c, n_chunks, [&](uint32_t ch) {
        const uint32_t t0 = ch * per, t1 = std::min<uint32_t>(n_tiles, t0 + per);
        const uint64_t S_lo = (uint64_t)t0 * TS, S_hi = (uint64_t)t1 * TS;
        const uint64_t off_lo = fe == FE_PIXELS ? S_lo / 13 * 18 : S_lo / 26 * 27;   // input bytes in front of the chunk (exact: S_lo is a multiple of the unit)
        const uint64_t up_hi = t1 == n_tiles ? in_bytes : std::min<uint64_t>(in_bytes, fe == FE_PIXELS ? S_hi / 13 * 18 : S_hi / 26 * 27);
        if (up_hi > up_done) { const hipError_t er = hipMemcpyAsync((uint8_t*)di + up_done, (const uint8_t*)in + up_done, up_hi - up_done, hipMemcpyHostToDevice, c.stream); if (er != hipSuccess) return fail_hip(er, "hipMemcpyAsync(chunk upload)"); up_done = up_hi; }
        EncLaunch e = e0;
        const uint64_t u_lo = off_lo / UB;                                            // pixels / words in front of the chunk
        e.a.in += off_lo;
        e.a.n_units = n_units > u_lo ? n_units - u_lo : 0; e.a.n_units_pad -= u_lo;
        e.a.n_sym = (uint32_t)(L.n_sym > S_lo ? L.n_sym - S_lo : 0);
        e.a.n_tiles = t1 - t0;
        fill_bands(e.a, L, (uint64_t)t0 * nb);
        if (ch) e.a.frame_out = nullptr;                                              // header and pad: the first chunk's first workgroup
        std::lock_guard<std::mutex> lk(c.mu);
        return launch_enc(c, e, c.stream);
    }, [&](uint32_t ch, hipStream_t s2) {
        const uint64_t t0 = (uint64_t)ch * per, t1 = std::min<uint64_t>(n_tiles, t0 + per);
        hipError_t er = copy_band_runs(ho, dob, L, hs, t0 * nb, t1 * nb, allow_strided, hipMemcpyDeviceToHost, s2);
        if (ch == 0 && er == hipSuccess) {                                          // header and the zero tail of the last word: written by the first chunk's first workgroup
            er = hipMemcpyAsync(ho, dob, hs, hipMemcpyDeviceToHost, s2);
            const uint64_t tail = 9 * L.out_words - (hs + L.body_syms);
            if (er == hipSuccess && tail) er = hipMemcpyAsync(ho + hs + L.body_syms, dob + hs + L.body_syms, tail, hipMemcpyDeviceToHost, s2);
        }
        return er;
    });
}

static int encode_host(int fe, const void* in, uint64_t n_units, const t3_cfg* cfg, void* out, uint64_t cap, uint64_t* n_out) {
    Ctx& c = ctx(); if (!c.ready) return T3_E_NODEVICE;
    if (!cfg || !n_out || (n_units && !in)) return T3_E_ARG;
    const uint64_t n_raw = fe == FE_PIXELS ? (n_units + 1) / 2 : n_units;
    t3_layout L; int rc = plan(n_raw, *cfg, L); if (rc) return rc;
    *n_out = L.out_words; if (L.out_words > cap) return T3_E_CAPACITY;
    std::lock_guard<std::recursive_mutex> hl(c.host_mu);
    void *di, *dout;
    rc = scratch(c, Scratch::HostIn, n_units * (fe == FE_PIXELS ? 6 : 9) + 64, &di); if (rc) return rc;
    rc = scratch(c, Scratch::HostOut, L.out_words * 9 + 64, &dout); if (rc) return rc;
    rc = encode_host_pipelined(c, fe, in, n_units, cfg, out, L, di, dout);                 // 1: not this framing / too small -> one upload, one launch, one download
    if (rc != 1) return rc;
    if (n_units) HIPCHK(hipMemcpyAsync(di, in, n_units * (fe == FE_PIXELS ? 6 : 9), hipMemcpyHostToDevice, c.stream));
    rc = encode_dev(fe, di, n_units, cfg, dout, L.out_words, n_out, c.stream); if (rc) return rc;
    if (L.out_words) HIPCHK(hipMemcpyAsync(out, dout, L.out_words * 9, hipMemcpyDeviceToHost, c.stream));
    HIPCHK(hipStreamSynchronize(c.stream)); return T3_OK;
}
int t3hip_encode_profile(const void* raw, uint64_t n_raw, const t3_cfg* cfg, void* out, uint64_t cap, uint64_t* n_out) { return encode_host(FE_WORDS, raw, n_raw, cfg, out, cap, n_out); }
int t3hip_encode_frame(const void* px, uint64_t n_px, const t3_cfg* cfg, void* out, uint64_t cap, uint64_t* n_out) { return encode_host(FE_PIXELS, px, n_px, cfg, out, cap, n_out); }

// ---- batches of equal frames ---------------------------------------------------------------------------------
int t3hip_frames_plan(int decode, uint64_t n_units, uint32_t n_frames, const t3_cfg* cfg, int fmt, t3_frames_plan* out) {
    if (!cfg || !out) return T3_E_ARG;
    t3_layout L; return plan_frames(decode, n_units, n_frames, *cfg, fmt, *out, L);
}
int t3hip_encode_frames_dev(const void* d_in, uint64_t n_units, int in_fmt, uint64_t in_stride, uint32_t n_frames, const t3_cfg* cfg, void* d_out, uint64_t out_stride,
                            uint64_t* n_out_words, void* stream) {
    return encode_frames_dev(d_in, n_units, in_fmt, in_stride, n_frames, cfg, d_out, out_stride, n_out_words, (hipStream_t)stream);
}
int t3hip_encode_frames(const void* in, uint64_t n_units, int in_fmt, uint64_t in_stride, uint32_t n_frames, const t3_cfg* cfg, void* out, uint64_t out_stride,
                        uint64_t* n_out_words) {
    Ctx& c = ctx(); if (!c.ready) return T3_E_NODEVICE;
    if (!cfg || !n_out_words || (n_frames && n_units && !in)) return T3_E_ARG;
    t3_frames_plan fp; t3_layout L;
    int rc = plan_frames(0, n_units, n_frames, *cfg, in_fmt, fp, L); if (rc) return rc;
    *n_out_words = L.out_words;
    if (n_frames == 0) return T3_OK;
    if (fp.out_bytes && !out) return T3_E_ARG;
    if (n_frames == 1) { in_stride = fp.in_stride_min; out_stride = fp.out_stride_min; }
    else if (!frames_strides_ok(fp, nullptr, in_stride, nullptr, out_stride)) return T3_E_ARG;
    std::lock_guard<std::recursive_mutex> hl(c.host_mu);
    void *di, *dout;
    rc = scratch(c, Scratch::HostIn, (uint64_t)n_frames * in_stride + 64, &di); if (rc) return rc;
    rc = scratch(c, Scratch::HostOut, (uint64_t)n_frames * out_stride + 64, &dout); if (rc) return rc;
    HIPCHK(copy_frames(di, in, in_stride, fp.in_bytes, n_frames, hipMemcpyHostToDevice, c.stream));
    rc = encode_frames_dev(di, n_units, in_fmt, in_stride, n_frames, cfg, dout, out_stride, n_out_words, c.stream); if (rc) return rc;
    HIPCHK(copy_frames(out, dout, out_stride, fp.out_bytes, n_frames, hipMemcpyDeviceToHost, c.stream));
    HIPCHK(hipStreamSynchronize(c.stream)); return T3_OK;
}

}  // extern "C"
