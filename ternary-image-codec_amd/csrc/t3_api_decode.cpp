// t3_api_decode.cpp — decode-side half of the C-ABI (include/t3hip.h): header parse on the host, body kernels
// on the device, block-level decode, error injector.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <stdlib.h>

#include <algorithm>
#include <mutex>
#include <vector>

#include "../../include/t3hip.h"
#include "t3_ctx.hpp"
#include "t3_dec_plan.hpp"
#include "t3_decode.h"
#include "t3_host.hpp"
#include "t3_repair.h"
#include "t3_window.h"

using namespace t3;

namespace {
// The streaming entry's header check (t3hip_decode_frame_async): the header symbols its configuration encodes to, how many, the verdict
// words and the frame.  decode_body settles it once, in front of the body decode: inside a one-launch decoder's launch (settle_header) or
// by hdr_compare_kernel -- either way before anything counts failures into verdict[1].
struct HdrCheck { HdrExpect ex; uint32_t hs; uint32_t* verdict; const uint8_t* in; };

int launch_hdr_compare(const HdrCheck* h, hipStream_t s) {           // h == nullptr: no check
    if (!h) return T3_OK;
    hipLaunchKernelGGL(hdr_compare_kernel, dim3(1), dim3(128), 0, s, h->in, h->ex, h->hs, h->verdict);   // also zeroes the block counter
    HIPCHK(hipGetLastError());
    return T3_OK;
}
// The header check and the verdict words in the launch of a one-launch decoder (DecFx2Args / DecUepArgs) that has tile tickets (the
// workgroup that finishes last knows it) and covers the whole frame, for a header of at most 96 symbols at a 4-byte aligned address;
// else hdr_compare_kernel in front of it
template <class A> int settle_header(A& a, const HdrCheck* h, bool whole_frame, hipStream_t s) {
    static const bool no_fold = getenv("T3HIP_HDR_KERNEL") != nullptr;                    // measurement / test knob: the separate header kernel
    if (!h || !a.tile_ctr || !whole_frame || no_fold || h->hs > 96u || ((uintptr_t)h->in & 3u) != 0) return launch_hdr_compare(h, s);
    a.verdict = h->verdict; a.hdr_in = h->in; a.hdr_n = h->hs; memcpy(a.hx, h->ex.b, 96);
    a.fail = a.tile_ctr + 64u * a.n_classes + 16u;                                        // library-owned, zero between launches; the last workgroup moves it to verdict[1]
    return T3_OK;
}

// The lazily built device tables below are shared by every caller thread of a context, and so are the pinned host mailboxes of the
// synchronous entry points: both locks live in the context (Ctx::tab_mu / Ctx::mail_mu), two contexts never share one.

// device tables of one code (syndrome LUT, root masks) and the multiply-accumulate table, built on first use (caller holds tab_mu)
int ensure_fx_tables(DecodeTables& tab, int k) {
    const int ki = k_index(k);
    if (!tab.synd_lut[ki]) {
        std::vector<uint32_t> img; build_syndrome_lut(k, img);
        HIPCHK(hipMalloc((void**)&tab.synd_lut[ki], img.size() * 4u));
        HIPCHK(hipMemcpy(tab.synd_lut[ki], img.data(), img.size() * 4u, hipMemcpyHostToDevice));
    }
    if (!tab.roots[ki]) {
        // sigma_0 = 1 always (Berlekamp-Massey), so sigma is its t = r/2 higher coefficients: 27^t locators (80 KB for
        // RS(26,20), 2 MB for RS(26,18)).  Entry = the 26-bit mask of positions i with sigma(alpha^-i) = 0.
        const Field& F = field(); const int t = (26 - k) / 2;
        size_t n = 1; for (int i = 0; i < t; ++i) n *= 27;
        std::vector<uint32_t> tbl(n);
        for (size_t idx = 0; idx < n; ++idx) {
            uint8_t sg[5] = {1, 0, 0, 0, 0}; { size_t v = idx; for (int q = 1; q <= t; ++q) { sg[q] = (uint8_t)(v % 27); v /= 27; } }
            uint32_t mask = 0;
            for (int i = 0; i < 26; ++i) {
                const uint8_t x = F.t.exp[i == 0 ? 0 : 26 - i];
                uint8_t acc = sg[t];
                for (int q = t - 1; q >= 0; --q) acc = F.t.add[F.t.mul[acc * 27 + x] * 27 + sg[q]];
                if (acc == 0) mask |= 1u << i;
            }
            tbl[idx] = mask;
        }
        HIPCHK(hipMalloc((void**)&tab.roots[ki], n * 4));
        HIPCHK(hipMemcpy(tab.roots[ki], tbl.data(), n * 4, hipMemcpyHostToDevice));
    }
    if (!tab.synd_afrag[ki]) {
        std::vector<uint32_t> af; build_mfma_syndrome(k, af);
        HIPCHK(hipMalloc((void**)&tab.synd_afrag[ki], af.size() * 4)); HIPCHK(hipMemcpy(tab.synd_afrag[ki], af.data(), af.size() * 4, hipMemcpyHostToDevice));
    }
    if (!tab.synd_T) {
        std::vector<uint32_t> img; build_syndrome_T(img);
        HIPCHK(hipMalloc((void**)&tab.synd_T, img.size() * 4)); HIPCHK(hipMemcpy(tab.synd_T, img.data(), img.size() * 4, hipMemcpyHostToDevice));
        build_syndrome_T(img, 16);
        HIPCHK(hipMalloc((void**)&tab.synd_T16, img.size() * 4)); HIPCHK(hipMemcpy(tab.synd_T16, img.data(), img.size() * 4, hipMemcpyHostToDevice));
        uint8_t sm[kFx2SmallBytes + kFx2ModBytes]; build_fx2_small(sm); build_fx2_mod(sm + kFx2SmallBytes);
        HIPCHK(hipMalloc((void**)&tab.fx2_small, sizeof sm)); HIPCHK(hipMemcpy(tab.fx2_small, sm, sizeof sm, hipMemcpyHostToDevice));
    }
    if (!tab.fma) {
        const Field& F = field();
        std::vector<uint8_t> t(kFmaBytes, 0);
        for (int x = 0; x < 27; ++x) for (int y = 0; y < 27; ++y) for (int c = 0; c < 27; ++c) t[(size_t)(x * 27 + y) * 27 + c] = F.t.add[c * 27 + F.t.mul[x * 27 + y]];
        HIPCHK(hipMalloc((void**)&tab.fma, t.size())); HIPCHK(hipMemcpy(tab.fma, t.data(), t.size(), hipMemcpyHostToDevice));
    }
    return T3_OK;
}

// dequantiser tables of the fused RGB output stage (old/include/io_image.hpp:79-84: the reference's double expressions, tabulated)
int rgb_dequant_tables(Ctx& c, const uint8_t** out) {                 // caller holds c.tab_mu
    uint8_t*& d = c.rgb.dequant;
    if (!d) {
        uint8_t t[328]; memset(t, 0, sizeof t);
        auto cl = [](long v) { return v < 0 ? 0 : (v > 255 ? 255 : v); };
        for (int q = 0; q <= 242; ++q) t[q] = (uint8_t)cl(lround(q * (255.0 / 242.0)));
        for (int q = -40; q <= 40; ++q) t[244 + q + 40] = (uint8_t)cl(lround(128 + q * (128.0 / 40.0)));
        HIPCHK(hipMalloc((void**)&d, sizeof t)); HIPCHK(hipMemcpy(d, t, sizeof t, hipMemcpyHostToDevice));
    }
    *out = d; return T3_OK;
}

// The FIXED decoders come in three steps: plan_* (t3_dec_plan.cpp, host arithmetic) fills the kernel arguments, or returns 1 when the framing
// is not its own; bind_* builds the lazily made tables under tab_mu, attaches their addresses and the caller's pointers, picks the kernel the
// plan names and sizes the grid; launch_* runs the plan on `body`, the coded stream, and settles the header check `hdr` first.
// the tables of every group's code built under tab_mu; attach(group, k index) takes the addresses the kernel reads
template <class A, class F> int bind_groups(Ctx& c, A& a, F attach) {
    std::lock_guard<std::mutex> lk(c.tab_mu);
    for (uint32_t g = 0; g < a.n_grp; ++g) { const int k = 26 - (int)a.grp[g].r; const int rc = ensure_fx_tables(c.dec, k); if (rc) return rc; attach(a.grp[g], k_index(k)); }
    a.fma = c.dec.fma; return T3_OK;
}
int bind_uep(UepPlan& p, void* d_out, uint32_t* d_fail) {
    Ctx& c = ctx(); DecUepArgs& a = p.a;
    { const int rc = bind_groups(c, a, [&](DecUepArgs::Grp& G, int ki) { G.afrag = c.dec.synd_afrag[ki]; G.roots = c.dec.roots[ki]; a.ttab = c.dec.synd_T16; a.small = c.dec.fx2_small; }); if (rc) return rc; }
    a.out = d_out; a.fail = d_fail;
    p.fn = by_r(p.ra, [&](auto A) { return by_r(p.rb, [&](auto B) -> const void* {      // instantiated for ra >= rb, as the plan orders the groups
        if constexpr (decltype(A)::value >= decltype(B)::value) return (const void*)decode_uep_px_kernel<decltype(A)::value, decltype(B)::value>; else return nullptr; }); });
    if (!p.fn) return T3_E_ARG;
    return resident_grid(c, p.fn, 512, a.lds_bytes, a.n_tiles, true, &p.grid);
}
int bind_stream(StreamPlan& p, void* d_out, uint32_t* d_fail) {
    Ctx& c = ctx(); DecStArgs& a = p.a;
    { const int rc = bind_groups(c, a, [&](DecStArgs::Grp& G, int ki) { G.lut = c.dec.synd_lut[ki]; G.roots = c.dec.roots[ki]; a.tab = c.dec.fxtab; }); if (rc) return rc; }
    a.fail = d_fail; p.e.out = d_out;
    p.emit_fn = p.to_pixels ? (const void*)emit_stream_kernel<true> : (const void*)emit_stream_kernel<false>;
    { const int rc = resident_grid(c, (const void*)decode_stream_kernel, 512, a.lds_bytes, a.n_tiles, false, &p.grid); if (rc) return rc; }
    return resident_grid(c, p.emit_fn, 512, p.e.lds_bytes, p.e.n_steps, false, &p.emit_grid);
}

int launch_fixed_fused(FusedPlan& p, const uint8_t* body, const HdrCheck* hdr, hipStream_t s) {
    Ctx& c = ctx(); DecFx2Args& a = p.a; const uint32_t grid = p.grid;
    a.in = body;
#ifdef T3_DEC_STAMPS
    static uint64_t* d_dbg = nullptr; static int calls = 0;
    if (!d_dbg) HIPCHK(hipMalloc((void**)&d_dbg, 16 * 8 * 4096));
    HIPCHK(hipMemsetAsync(d_dbg, 0, 16 * 8 * 4096, s));
    a.dbg = d_dbg;
#endif
    if (p.tickets) tile_tickets(c, s, 1, grid, &a.tile_ctr, &a.n_classes);     // dynamic tile tickets (decode_fixed_px_kernel)
    { const int rc = settle_header(a, hdr, p.whole_frame, s); if (rc) return rc; }
    void* args[] = {(void*)&a};
    HIPCHK(hipLaunchKernel(p.fn, dim3(grid), dim3(p.threads), args, a.lds_bytes, s));
#ifdef T3_DEC_STAMPS
    if (++calls == 8 && p.tickets) {                        // one report, after warm-up: mean cycles of waves 0 / 4 per workgroup and phase
        std::vector<uint64_t> h(16 * grid);
        HIPCHK(hipStreamSynchronize(s));
        HIPCHK(hipMemcpy(h.data(), d_dbg, h.size() * 8, hipMemcpyDeviceToHost));
        double acc[16] = {0};
        for (uint32_t w = 0; w < grid; ++w) for (int i = 0; i < 16; ++i) acc[i] += (double)h[16 * w + i];
        fprintf(stderr, "[t3 dec stamps] grid=%u (%d per CU) tiles=%u lds=%u  mean cycles/WG: producer sets+e1=%.0f barrier=%.0f total=%.0f | consumer bm=%.0f rendezvous=%.0f d5=%.0f barrier=%.0f total=%.0f  clock=%.3f GHz  us/WG=%.1f\n",
                grid, (int)((grid + c.n_cu - 1) / c.n_cu), a.n_tiles, a.lds_bytes, acc[0] / grid, acc[1] / grid, acc[6] / grid, acc[8 + 2] / grid, acc[8 + 3] / grid, acc[8 + 4] / grid, acc[8 + 5] / grid, acc[8 + 6] / grid,
                acc[6] / acc[7] * 0.1, acc[7] / grid * 0.01);
        uint64_t s0 = ~0ull, s1 = 0, e1 = 0; int late = 0;
        for (uint32_t w = 0; w < grid; ++w) { s0 = std::min(s0, h[16 * w + 2]); s1 = std::max(s1, h[16 * w + 2]); e1 = std::max(e1, h[16 * w + 3]); }
        for (uint32_t w = 0; w < grid; ++w) if (h[16 * w + 2] - s0 > 1000) ++late;
        fprintf(stderr, "[t3 dec stamps]   prologue (kernel entry -> first tile's input landed, wave 0): mean %.0f cycles/WG\n", acc[4] / grid);
        fprintf(stderr, "[t3 dec stamps]   timeline (us from first loop start): last start=%.1f last end=%.1f  workgroups starting >10 us late=%d\n", (s1 - s0) * 0.01, (e1 - s0) * 0.01, late);
    }
#endif
    return T3_OK;
}

// One launch for per-band k and / or the 2-D interleave, pixels out (t3_decode_uep.hip)
int launch_fixed_uep(UepPlan& p, const uint8_t* body, const HdrCheck* hdr, hipStream_t s) {
    Ctx& c = ctx(); DecUepArgs& a = p.a;
    void* d_e; int rc = scratch(c, Scratch::StreamWork, (size_t)a.n_sym + 64, &d_e, s); if (rc) return rc;
    a.in = body; a.edge = (uint8_t*)d_e;
    tile_tickets(c, s, 2, p.grid, &a.tile_ctr, &a.n_classes);
    rc = settle_header(a, hdr, true, s); if (rc) return rc;
    void* args[] = {(void*)&a};
    HIPCHK(hipLaunchKernel(p.fn, dim3(p.grid), dim3(512), args, a.lds_bytes, s));
    HIPCHK(hipLaunchKernel((const void*)uep_edge_kernel, dim3((3u * a.n_tiles + 1u + 255u) / 256u), dim3(256), args, 0, s));
    return T3_OK;
}

// Two kernels (t3_decode_stream.hip): any per-band k, 1-D or 2-D
int launch_fixed_stream(StreamPlan& p, const uint8_t* body, const HdrCheck* hdr, hipStream_t s) {
    void* d_y; int rc = scratch(ctx(), Scratch::StreamWork, (size_t)p.a.n_sym + 64, &d_y, s); if (rc) return rc;
    p.a.in = body; p.a.ystream = (uint8_t*)d_y; p.e.ystream = (const uint8_t*)d_y;
    rc = launch_hdr_compare(hdr, s); if (rc) return rc;
    void* args[] = {(void*)&p.a}; void* eargs[] = {(void*)&p.e};
    HIPCHK(hipLaunchKernel((const void*)decode_stream_kernel, dim3(p.grid), dim3(512), args, p.a.lds_bytes, s));
    HIPCHK(hipLaunchKernel(p.emit_fn, dim3(p.emit_grid), dim3(512), eargs, p.e.lds_bytes, s));
    return T3_OK;
}

// body decode with a known config (header already parsed); hdr: the streaming entry's header check (nullptr: none)
int decode_body(const void* d_in, uint64_t n_in, const t3_cfg& cfg, uint64_t n_raw, const uint8_t next[3],
                void* d_out, uint64_t cap_units, uint64_t* n_out, int to_pixels, uint32_t* d_fail, hipStream_t s, const HdrCheck* hdr) {
    const bool fixed = cfg.mode == T3_MODE_FIXED;
    // to_pixels == 2: RGB8 out (row f1 fused into the pixel decoder's output stage); only the fused FIXED kernel takes it, every
    // other framing answers 1 with nothing launched, and the caller converts a pixel scratch with the bridge kernel
    const bool want_rgb = to_pixels == 2;
    // t3hip.h: the coded stream and a pixel destination at an even address (the fused kernels read the stream as 2-byte aligned
    // granules, load16; pixel components are 16-bit); raw words and RGB go out at any address
    if (((uintptr_t)d_in & 1u) != 0 || (to_pixels == 1 && ((uintptr_t)d_out & 1u) != 0)) return T3_E_ARG;
    if (want_rgb && !fixed) return 1;
    Ctx& c = ctx();
    DecArgs a; memset(&a, 0, sizeof a);
    EmitArgs e; memset(&e, 0, sizeof e);
    a.in = (const uint8_t*)d_in; a.fail = d_fail; a.tab = c.d_tab; a.fixed = fixed ? 1 : 0;
    const ScrCycle sc = scrambler_cycle_from_next(next, cfg.seed_s0);
    a.cyc24 = sc.cyc24; a.pre0 = sc.pre[0]; a.pre1 = sc.pre[1];
    a.beacon_on = (cfg.beacon_enabled && cfg.beacon_words_period > 0) ? 1 : 0; a.period = cfg.beacon_words_period; a.slot = cfg.beacon_band_slot;
    uint64_t use_syms, n_words, total = 0;
    if (!fixed) {
        DecLayoutCompat D; plan_decode_compat(n_in, cfg, D);
        a.hdr_syms = 54;
        for (int b = 0; b < 9; ++b) { a.band_k[b] = D.band_k[b]; a.band_blocks[b] = D.band_blocks[b]; a.band_first[b] = total; a.band_off[b] = D.use_off[b]; total += D.band_blocks[b]; }
        use_syms = D.use_syms; n_words = D.out_words;
    } else {
        t3_layout L; int rc = plan(n_raw, cfg, L); if (rc) return T3_E_HEADER;
        if (L.out_words > n_in) return T3_E_HEADER;                      // truncated stream
        a.hdr_syms = 90; a.n_sym = L.n_sym;
        for (int b = 0; b < 9; ++b) { a.band_k[b] = L.band_k[b]; a.band_blocks[b] = L.band_blocks[b]; a.band_first[b] = total; a.band_off[b] = L.band_body_off[b]; total += L.band_blocks[b]; }
        use_syms = L.n_sym; n_words = n_raw;
        const uint64_t funits = want_rgb ? cap_units : to_pixels ? 2 * n_words : n_words;     // RGB: exactly the caller's pixel count (no pad pixel)
        if (want_rgb && (cap_units > 2 * n_words || cap_units + 1 < 2 * n_words || L.interleave2d)) return 1;
        if (want_rgb && !single_k(L)) return 1;
        if (funits <= cap_units && (!to_pixels || ((uintptr_t)d_out & 15u) == 0) && !generic_decode() && 9 * n_in < (1ull << 32)) {
            // The first decoder that plans the frame takes it, in this order: the fused kernel with a beacon stepped over in its loads;
            // then, on the body without its beacons (stripped by debeacon_kernel once the choice is made) or else the frame, the fused
            // kernel, the one-launch UEP / 2-D decoder (pixels), the two-kernel decoder.  Nothing is launched before the choice.
            const bool bcn_ok = L.beacon_on && cfg.beacon_band_slot < 9 && cfg.beacon_words_period >= 2 && cfg.beacon_words_period < (1u << 27) && getenv("T3HIP_BEACON_PASS") == nullptr;
            const uint64_t bytes = L.beacon_on ? L.body_syms : 9 * n_in; const uint32_t hs = L.beacon_on ? 0u : L.header_syms;
            FusedPlan fp; UepPlan up; StreamPlan sp;
            const FusedForm form = (FusedForm)to_pixels;
            int path = 0, frc = bcn_ok ? plan_fixed_fused(9 * n_in, L.header_syms, L, sc, funits, form, fp, cfg.beacon_band_slot, cfg.beacon_words_period)
                                       : plan_fixed_fused(bytes, hs, L, sc, funits, form, fp);
            if (frc == 1 && want_rgb) return 1;
            if (frc == 1 && to_pixels == 1) { path = 1; frc = plan_fixed_uep(bytes, hs, cfg, L, sc, funits, getenv("T3HIP_TWO_KERNEL_DECODE") != nullptr, up); }
            static const uint32_t lut_bytes[4] = {synd_lut_bytes(24), synd_lut_bytes(22), synd_lut_bytes(20), synd_lut_bytes(18)};
            if (frc == 1) { path = 2; frc = plan_fixed_stream(bytes, hs, cfg, L, sc, funits, to_pixels, lut_bytes, sp); }
            if (frc == T3_OK) frc = path == 0 ? bind_fused(fp, d_out, d_fail) : path == 1 ? bind_uep(up, d_out, d_fail) : bind_stream(sp, d_out, d_fail);
            if (frc < 0) return frc;
            if (frc == T3_OK) {
                const uint8_t* body = (const uint8_t*)d_in;
                if (L.beacon_on && !(path == 0 && bcn_ok)) {
                    void* d_b; int brc = scratch(c, Scratch::StreamBody, L.body_syms + 64, &d_b, s); if (brc) return brc;
                    DebeaconArgs d; d.framed = (const uint8_t*)d_in + L.header_syms; d.framed_bytes = 9 * n_in - L.header_syms; d.body = (uint8_t*)d_b; d.body_syms = L.body_syms; d.period = cfg.beacon_words_period; d.slot = cfg.beacon_band_slot;
                    if (L.body_syms) { hipLaunchKernelGGL(debeacon_kernel, dim3(blocks_for((L.body_syms + 15) / 16, 1u << 20)), dim3(256), 0, s, d); HIPCHK(hipGetLastError()); }
                    body = (const uint8_t*)d_b;
                }
                frc = path == 0 ? launch_fixed_fused(fp, body, hdr, s) : path == 1 ? launch_fixed_uep(up, body, hdr, s) : launch_fixed_stream(sp, body, hdr, s);
                if (frc == T3_OK) *n_out = funits;
                return frc;
            }
        }
    }
    if (want_rgb) return 1;
    a.total_blocks = total;
    const uint64_t units = to_pixels ? 2 * n_words : n_words;
    *n_out = units;
    if (units > cap_units) return T3_E_CAPACITY;
    void* d_use; int rc = scratch(c, Scratch::StreamWork, use_syms + 64, &d_use, s); if (rc) return rc;
    rc = launch_hdr_compare(hdr, s); if (rc) return rc;
    a.use = (uint8_t*)d_use;
    if (total) { hipLaunchKernelGGL(dec_gather_rs_kernel, dim3(blocks_for(total, 1u << 20)), dim3(256), 0, s, a); HIPCHK(hipGetLastError()); }
    e.use = (const uint8_t*)d_use; e.use_syms = use_syms; e.out = d_out; e.n_words = n_words; e.to_pixels = to_pixels ? 1 : 0;
    const bool il = cfg.profile == T3_P5_RS26_22_2D && cfg.tile_w && cfg.tile_h && use_syms;   // OLD:1018
    e.il_on = il ? 1 : 0;
    if (il) fill_interleave(e, cfg, use_syms);
    if (n_words) { hipLaunchKernelGGL(dec_emit_kernel, dim3(blocks_for(n_words, 1u << 20)), dim3(256), 0, s, e); HIPCHK(hipGetLastError()); }
    return T3_OK;
}

int read_header(const void* d_in, uint64_t n_in, int mode, t3_cfg* seen, uint64_t* n_raw, uint8_t next[3], hipStream_t s) {
    const uint64_t hw = mode == T3_MODE_FIXED ? 10 : 6;
    if (n_in < hw) return T3_E_HEADER;                                     // OLD:920
    // pinned mailbox: the 54/90 header bytes come back by a real asynchronous DMA (a pageable target costs a staging copy)
    Ctx& c = ctx();
    std::lock_guard<std::mutex> lk(c.mail_mu);
    uint8_t*& h = c.mail.header;
    if (!h) HIPCHK(hipHostMalloc((void**)&h, 128, hipHostMallocDefault));
    HIPCHK(hipMemcpyAsync(h, d_in, hw * 9, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    uint8_t hb[96]; memcpy(hb, h, hw * 9);
    return header_parse(hb, n_in, mode, *seen, n_raw, next);
}

// The crop of a decoded run (first_px on, 16-byte aligned) into the caller's window buffer; out_fmt 1: pixels, 2: RGB8.  The arguments of
// one frame's crop, shared by the two launches below; a.lead: the destination's address mod 16
int fill_window_crop(WinCropArgs& a, const void* d_run, uint64_t first_px, uint64_t stream_px, uint32_t fw, uint32_t fh, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                     void* d_out, bool rgb) {
    Ctx& c = ctx();
    memset(&a, 0, sizeof a);
    if (rgb) { std::lock_guard<std::mutex> lk(c.tab_mu); const int rc = rgb_dequant_tables(c, &a.dq); if (rc) return rc; }
    a.run = (const uint8_t*)d_run; a.out = (uint8_t*)d_out; a.first_px = first_px; a.stream_px = stream_px;
    a.out_bytes = (uint64_t)w * h * (rgb ? 3u : 6u);
    a.lead = (uint32_t)((uintptr_t)d_out & 15u); a.n_gran = (a.lead + a.out_bytes + 15u) / 16u;
    a.fw = fw; a.fh = fh; a.x0 = x0; a.y0 = y0; a.w = w; a.h = h;
    a.wide = a.out_bytes >= (1ull << 31) ? 1u : 0u;
    if (!a.wide) a.div_row = to_dev(fastdiv(rgb ? w : 3u * w)); else a.div_row.d = rgb ? w : 3u * w;
    return a.n_gran > (1ull << 38) || 3ull * w >= (1ull << 32) ? T3_E_ARG : T3_OK;
}
int launch_window_crop(const void* d_run, uint64_t first_px, uint64_t stream_px, uint32_t fw, uint32_t fh, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                       void* d_out, int out_fmt, hipStream_t s) {
    WinCropArgs a; const bool rgb = out_fmt == 2;
    { const int rc = fill_window_crop(a, d_run, first_px, stream_px, fw, fh, x0, y0, w, h, d_out, rgb); if (rc) return rc; }
    const void* fn = rgb ? (const void*)window_crop_kernel<true> : (const void*)window_crop_kernel<false>;
    void* args[] = {(void*)&a};
    HIPCHK(hipLaunchKernel(fn, dim3((unsigned)((a.n_gran + 255u) / 256u)), dim3(256), args, 0, s));
    return T3_OK;
}
// the same crop over the n_frames decoded runs of a batch in one launch (frame f: run + f * run_stride -> out + f * out_stride, both
// 16-byte aligned with strides that are multiples of 16: lead = 0)
int launch_window_crop_frames(const void* d_run, uint64_t run_stride, uint64_t first_px, uint64_t stream_px, uint32_t fw, uint32_t fh, uint32_t x0, uint32_t y0,
                              uint32_t w, uint32_t h, void* d_out, uint64_t out_stride, int out_fmt, uint32_t n_frames, hipStream_t s) {
    WinCropFramesArgs fa; memset(&fa, 0, sizeof fa);
    const bool rgb = out_fmt == 2;
    { const int rc = fill_window_crop(fa.a, d_run, first_px, stream_px, fw, fh, x0, y0, w, h, d_out, rgb); if (rc) return rc; }
    fa.run_stride = run_stride; fa.out_stride = out_stride;
    if (n_frames > 65535u || (((uintptr_t)d_run | (uintptr_t)d_out | run_stride | out_stride) & 15u)) return T3_E_ARG;
    const void* fn = rgb ? (const void*)window_crop_frames_kernel<true> : (const void*)window_crop_frames_kernel<false>;
    void* args[] = {(void*)&fa};
    HIPCHK(hipLaunchKernel(fn, dim3((unsigned)((fa.a.n_gran + 255u) / 256u), n_frames), dim3(256), args, 0, s));
    return T3_OK;
}

// ONE launch of dec_frames_px over a batch of equal frames, from the plan of frame 0 (bound here; d_out: where the plan's output starts):
// frame f is read in_stride behind, written out_stride behind, its header compared with the symbols cfg and n_raw encode to.  A batch the
// plan calls one launch runs as one launch or not at all (T3_E_ARG), never silently as the callers' loops.
int launch_fused_frames(FusedPlan& p, const void* d_in, uint64_t in_stride, void* d_out, uint64_t out_stride, uint32_t n_frames, const t3_cfg& cfg, uint64_t n_raw,
                        uint32_t* d_verdict, hipStream_t s) {
    uint8_t hx[96]; memset(hx, 0, sizeof hx);
    const uint32_t hs = (uint32_t)header_encode(cfg, n_raw, hx);
    if (!p.tickets || hs > 96u) return T3_E_ARG;
    { const int rc = bind_fused(p, d_out, nullptr, n_frames); if (rc) return rc; }
    DecFramesArgs fa; memset(&fa, 0, sizeof fa);
    fa.a = p.a; fa.a.in = (const uint8_t*)d_in; fa.a.verdict = d_verdict; fa.a.hdr_in = (const uint8_t*)d_in; fa.a.hdr_n = hs; memcpy(fa.a.hx, hx, 96);
    fa.in_stride = in_stride; fa.out_stride = out_stride; fa.n_frames = n_frames;
    fa.n_total = n_frames * fa.a.n_tiles; fa.div_tiles = to_dev(fastdiv(fa.a.n_tiles));
    tile_tickets(ctx(), s, 1, p.grid, &fa.a.tile_ctr, &fa.a.n_classes);
    // the verdict words start at zero: the kernel writes every frame's header word and counts uncorrectable blocks into the other
    HIPCHK(hipMemsetAsync(d_verdict, 0, 8ull * n_frames, s));
    void* args[] = {(void*)&fa};
    HIPCHK(hipLaunchKernel(p.fn, dim3(p.grid), dim3(p.threads), args, fa.a.lds_bytes, s));
    return T3_OK;
}
}  // namespace

namespace t3 {
int decode_init(DecodeTables& tab) {   // field tables of the fused decoder
    const Field& F = field();
    static const uint8_t want_exp[26] = {1, 3, 9, 5, 15, 23, 13, 17, 20, 4, 12, 14, 11, 2, 6, 18, 7, 21, 16, 26, 22, 10, 8, 24, 25, 19};
    if (memcmp(F.t.exp, want_exp, 26) != 0) return T3_E_ARG;              // kExp in t3_decode_fused.hip is this table
    FxTables T; memset(&T, 0, sizeof T);
    memcpy(T.mul, F.t.mul, 729); memcpy(T.add, F.t.add, 729); memcpy(T.inv, F.t.inv, 27); memcpy(T.neg, F.t.neg, 27); memcpy(T.exp, F.t.exp, 26);
    for (int x = 0; x < 27; ++x) for (int y = 0; y < 27; ++y) T.sub[x * 27 + y] = F.t.add[x * 27 + F.t.neg[y]];
    for (int st = 0; st < 3; ++st) for (int c = 0; c < 27; ++c) T.descr[st][c] = (uint8_t)(4 * F.t.add[c * 27 + F.t.neg[13 * st]]);
    HIPCHK(hipMalloc((void**)&tab.fxtab, sizeof T));
    HIPCHK(hipMemcpy(tab.fxtab, &T, sizeof T, hipMemcpyHostToDevice));
    return T3_OK;
}
// The bind step of a planned fused launch (t3_ctx.hpp): the tables of the plan's k built and attached under tab_mu, d_out and d_fail, the
// kernel -- fn, else the decoder the plan names, its batch form for n_frames > 0 -- and its resident grid over the tiles of all frames
int bind_fused(FusedPlan& p, void* d_out, uint32_t* d_fail, uint32_t n_frames, const void* fn) {
    Ctx& c = ctx(); DecFx2Args& a = p.a; const int ki = k_index((int)a.k); const auto kv = p.kern;
    {
        std::lock_guard<std::mutex> lk(c.tab_mu);
        { const int rc = ensure_fx_tables(c.dec, (int)a.k); if (rc) return rc; }
        a.roots = c.dec.roots[ki]; a.ttab = (kv.px && T3_DEC_PX_TCOP == 16) ? c.dec.synd_T16 : c.dec.synd_T; a.small = c.dec.fx2_small; a.afrag = c.dec.synd_afrag[ki]; a.fma = c.dec.fma;
        if (kv.rgb) { const int rc = rgb_dequant_tables(c, &a.dq); if (rc) return rc; }
    }
    a.out = (uint8_t*)d_out + p.out_off; a.fail = d_fail;
    if (!fn) fn = by_r(kv.r, [&](auto R) -> const void* {
        constexpr int r = decltype(R)::value;
        if (n_frames) return kv.rgb ? (const void*)dec_frames_px<r, true, false> : (const void*)dec_frames_px<r, false, false>;      // t3_decode_frames.hip instantiates every one
        if (!kv.px) return kv.bcn ? (const void*)decode_fixed_kernel<r, true> : (const void*)decode_fixed_kernel<r, false>;
        if (kv.rgb) return kv.bcn ? (const void*)decode_fixed_px_kernel<r, true, true> : (const void*)decode_fixed_px_kernel<r, true, false>;
        return kv.bcn ? (const void*)decode_fixed_px_kernel<r, false, true> : (const void*)decode_fixed_px_kernel<r, false, false>;
    });
    p.fn = fn;
    return resident_grid(c, fn, (int)p.threads, a.lds_bytes, (uint64_t)std::max(n_frames, 1u) * a.n_tiles, true, &p.grid);
}
int decode_body_known(const void* d_in, uint64_t n_in, const t3_cfg& cfg, uint64_t n_raw, const uint8_t next[3], void* d_out, uint64_t cap_units,
                      uint64_t* n_out, int fmt, uint32_t* d_fail, hipStream_t s) {
    int rc = decode_body(d_in, n_in, cfg, n_raw, next, d_out, cap_units, n_out, fmt, d_fail, s, nullptr);
    if (rc != 1 || fmt != 2) return rc;
    void* d_q; rc = scratch(ctx(), Scratch::StreamRgb, 12 * n_raw + 64, &d_q, s); if (rc) return rc;
    rc = decode_body(d_in, n_in, cfg, n_raw, next, d_q, 2 * n_raw, n_out, 1, d_fail, s, nullptr); if (rc) return rc;
    *n_out = std::min<uint64_t>(cap_units, 2 * n_raw);
    return t3hip_quant_to_rgb_dev(d_q, *n_out, (uint8_t*)d_out, s);
}
int decode_window_known(const void* d_in, uint64_t n_in, const t3_cfg& cfg, uint64_t n_raw, const uint8_t next[3], uint32_t fw, uint32_t fh, uint32_t x0, uint32_t y0,
                        uint32_t w, uint32_t h, void* d_out, int out_fmt, uint32_t* d_fail, hipStream_t s) {
    const uint64_t units = 2 * n_raw;
    void* d_px; { const int rc = scratch(ctx(), Scratch::StreamWindow, 6 * units + 256, &d_px, s); if (rc) return rc; }
    uint64_t n_units = 0;
    { const int rc = decode_body_known(d_in, n_in, cfg, n_raw, next, d_px, units, &n_units, 1, d_fail, s); if (rc) return rc < 0 ? rc : T3_E_ARG; }
    return launch_window_crop(d_px, 0, std::min(n_units, units), fw, fh, x0, y0, w, h, d_out, out_fmt, s);
}
}  // namespace t3

extern "C" {

int t3hip_read_header_dev(const void* d_in, uint64_t n_in, int mode, t3_cfg* out_cfg, uint64_t* n_raw, void* stream) {
    if (!ctx().ready) return T3_E_NODEVICE;
    if (!out_cfg || (n_in && !d_in)) return T3_E_ARG;
    uint8_t next[3];
    return read_header(d_in, n_in, mode, out_cfg, n_raw, next, (hipStream_t)stream);
}

int t3hip_decode_body_dev(const void* d_in, uint64_t n_in, const t3_cfg* cfg, uint64_t n_raw, void* d_out, uint64_t cap, uint64_t* n_out,
                          int to_pixels, uint32_t* d_fail, void* stream) {
    if (!ctx().ready) return T3_E_NODEVICE;
    if (!cfg || !n_out || !d_fail) return T3_E_ARG;
    const ScrCycle sc = scrambler_cycle(cfg->seed_a, cfg->seed_b, cfg->seed_s0);
    return decode_body(d_in, n_in, *cfg, n_raw, sc.next, d_out, cap, n_out, to_pixels, d_fail, (hipStream_t)stream, nullptr);
}

int t3hip_decode_frame_async(const void* d_in, uint64_t n_in, const t3_cfg* cfg, uint64_t n_raw, void* d_out, uint64_t cap, uint64_t* n_out,
                             int to_pixels, uint32_t* d_verdict, void* stream) {
    if (!ctx().ready) return T3_E_NODEVICE;
    if (!cfg || !n_out || !d_verdict || (n_in && !d_in) || cfg->profile == T3_RAW_MODE) return T3_E_ARG;
    t3_layout L; int rc = plan(n_raw, *cfg, L); if (rc) return rc;
    // the expected header symbols travel as a kernel argument (96 bytes): nothing to allocate, no limit on how many different
    // headers a long-lived process may see
    HdrCheck h; memset(&h, 0, sizeof h);
    h.hs = (uint32_t)header_encode(*cfg, n_raw, h.ex.b); h.verdict = d_verdict; h.in = (const uint8_t*)d_in;
    if (9 * n_in < h.hs) return T3_E_HEADER;
    const ScrCycle sc = scrambler_cycle(cfg->seed_a, cfg->seed_b, cfg->seed_s0);
    return decode_body(d_in, n_in, *cfg, n_raw, sc.next, d_out, cap, n_out, to_pixels, d_verdict + 1, (hipStream_t)stream, &h);
}

// ---- batches of equal frames (t3hip.h): one launch of the fused pixel decoder over the tile space of all frames where it serves a frame,
// else a loop of the single-frame streaming entries
int t3hip_decode_frames_async(const void* d_in, uint64_t n_in, uint64_t in_stride, uint32_t n_frames, const t3_cfg* cfg, uint64_t n_raw, void* d_out, uint64_t out_stride,
                              int out_fmt, uint32_t* d_verdict, void* stream) {
    // what can be refused without a device is refused first: a null base never reaches a launch (0 is 16-byte aligned)
    if (!cfg || (n_frames && !d_verdict)) return T3_E_ARG;
    hipStream_t s = (hipStream_t)stream;
    t3_frames_plan fp; t3_layout L;
    const uint64_t units = out_fmt == 0 ? n_raw : 2 * n_raw;
    int rc = plan_frames(1, units, n_frames, *cfg, out_fmt, fp, L); if (rc) return rc;
    if (n_frames && ((n_in && !d_in) || (units && !d_out))) return T3_E_ARG;
    if (n_frames > 1 && !frames_strides_ok(fp, d_in, in_stride, d_out, out_stride)) return T3_E_ARG;
    Ctx& c = ctx(); if (!c.ready) return T3_E_NODEVICE;
    if (n_frames == 0) return T3_OK;
    if (fp.one_launch) {
        if (L.out_words > n_in) return T3_E_HEADER;                                  // truncated streams (decode_body)
        const ScrCycle sc0 = scrambler_cycle(cfg->seed_a, cfg->seed_b, cfg->seed_s0), sc = scrambler_cycle_from_next(sc0.next, cfg->seed_s0);
        // a frame's stream is its L.out_words words, whatever lies behind them in the stride (the plan bounds 9 * out_words by 2^32)
        FusedPlan p; rc = plan_fixed_fused(9 * L.out_words, L.header_syms, L, sc, units, (FusedForm)out_fmt, p);
        if (rc) return rc < 0 ? rc : T3_E_ARG;
        return launch_fused_frames(p, d_in, in_stride, d_out, out_stride, n_frames, *cfg, n_raw, d_verdict, s);
    }
    for (uint32_t f = 0; f < n_frames; ++f) {
        const uint8_t* in = (const uint8_t*)d_in + (uint64_t)f * in_stride; uint8_t* out = (uint8_t*)d_out + (uint64_t)f * out_stride; uint64_t n = 0;
        rc = out_fmt == 2 ? t3hip_decode_rgb_async(in, n_in, cfg, units, out, d_verdict + 2 * f, stream)
                          : t3hip_decode_frame_async(in, n_in, cfg, n_raw, out, units, &n, out_fmt, d_verdict + 2 * f, stream);
        if (rc) return rc;
    }
    return T3_OK;
}

int t3hip_window_plan(uint64_t n_raw, const t3_cfg* cfg, uint32_t fw, uint32_t fh, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, t3_window_plan* out) {
    if (!cfg || !out) return T3_E_ARG;
    t3_layout L;
    return plan_window(n_raw, *cfg, fw, fh, x0, y0, w, h, generic_decode(), *out, L);
}

// A w x h window of a coded frame: the tiles its rows live in (or the frame, for a framing without a tile range) decoded into a per-stream
// scratch, then window_crop_kernel.  d_verdict as for t3hip_decode_frame_async; the block counter sees the decoded blocks only.
int t3hip_decode_window_async(const void* d_in, uint64_t n_in, const t3_cfg* cfg, uint64_t n_raw, uint32_t fw, uint32_t fh, uint32_t x0, uint32_t y0,
                              uint32_t w, uint32_t h, void* d_out, int out_fmt, uint32_t* d_verdict, void* stream) {
    Ctx& c = ctx(); if (!c.ready) return T3_E_NODEVICE;
    if (!cfg || !d_verdict || (n_in && !d_in) || (out_fmt != 1 && out_fmt != 2)) return T3_E_ARG;
    t3_window_plan wp; t3_layout L;
    int rc = plan_window(n_raw, *cfg, fw, fh, x0, y0, w, h, generic_decode(), wp, L); if (rc) return rc;
    if ((uint64_t)w * h == 0) return T3_OK;
    if (!d_out || ((uintptr_t)d_out & 3u) || ((uintptr_t)d_in & 1u)) return T3_E_ARG;   // (d_in9 as for t3hip_decode_frame_async)
    hipStream_t s = (hipStream_t)stream;
    const uint64_t units = 2 * n_raw;
    if (!wp.tile_range || 9 * n_in >= (1ull << 32)) {                       // the whole frame, by the streaming entry, then the crop
        void* d_px; rc = scratch(c, Scratch::StreamWindow, 6 * units + 256, &d_px, s); if (rc) return rc;
        uint64_t n_units = 0;
        rc = t3hip_decode_frame_async(d_in, n_in, cfg, n_raw, d_px, units, &n_units, 1, d_verdict, stream); if (rc) return rc;
        return launch_window_crop(d_px, 0, std::min(n_units, units), fw, fh, x0, y0, w, h, d_out, out_fmt, s);
    }
    if (L.out_words > n_in) return T3_E_HEADER;                             // truncated stream (decode_body)
    HdrCheck hc; memset(&hc, 0, sizeof hc);
    hc.hs = (uint32_t)header_encode(*cfg, n_raw, hc.ex.b); hc.verdict = d_verdict; hc.in = (const uint8_t*)d_in;
    if (9 * n_in < hc.hs) return T3_E_HEADER;
    void* d_px; rc = scratch(c, Scratch::StreamWindow, 6 * wp.n_px + 256, &d_px, s); if (rc) return rc;
    if (wp.tile_hi > wp.tile_lo) {
        const ScrCycle sc = scrambler_cycle(cfg->seed_a, cfg->seed_b, cfg->seed_s0);
        // the decoder addresses its output by stream pixel: hand it the address pixel 0 would have (a tile starts on a multiple of 16 bytes)
        uint8_t* const base0 = (uint8_t*)((uintptr_t)d_px - (uintptr_t)(6 * wp.first_px));
        const bool all = wp.tile_lo == 0 && wp.tile_hi == wp.n_tiles;
        FusedPlan fp;
        rc = plan_fixed_fused(9 * n_in, L.header_syms, L, sc, wp.first_px + wp.n_px, FusedForm::Pixels, fp, 0, 0, all ? 0u : wp.tile_lo, all ? 0xFFFFFFFFu : wp.tile_hi);
        if (rc) return rc == 1 ? T3_E_ARG : rc;                             // (plan_window chose this path for the framing plan_fixed_fused takes)
        rc = bind_fused(fp, base0, d_verdict + 1); if (rc) return rc;
        rc = launch_fixed_fused(fp, (const uint8_t*)d_in, &hc, s); if (rc) return rc;
    } else { rc = launch_hdr_compare(&hc, s); if (rc) return rc; }           // no tile: the header verdict, a zero block count, a zero window
    return launch_window_crop(d_px, wp.first_px, units, fw, fh, x0, y0, w, h, d_out, out_fmt, s);
}

int t3hip_frames_window_plan(uint64_t n_raw, uint32_t n_frames, const t3_cfg* cfg, uint32_t fw, uint32_t fh, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                             int out_fmt, t3_frames_window_plan* out) {
    if (!cfg || !out) return T3_E_ARG;
    t3_layout L;
    return plan_frames_window(n_raw, n_frames, *cfg, fw, fh, x0, y0, w, h, out_fmt, generic_decode(), *out, L);
}

// The same window out of every frame of a batch.  One launch: the fused pixel decoder over the tile range of all frames (dec_frames_px on
// a DecFramesArgs built around the tile-range plan: the kernel sees n_frames frames of tile_hi - tile_lo tiles each) into a per-stream
// scratch, one run per frame, then one crop launch over the runs.  Else a loop of t3hip_decode_window_async.
int t3hip_decode_frames_window_async(const void* d_in, uint64_t n_in, uint64_t in_stride, uint32_t n_frames, const t3_cfg* cfg, uint64_t n_raw, uint32_t fw, uint32_t fh,
                                     uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, void* d_out, uint64_t out_stride, int out_fmt, uint32_t* d_verdict, void* stream) {
    // what can be refused without a device is refused first: a null base never reaches a launch (0 is 16-byte aligned)
    if (!cfg || (n_frames && !d_verdict)) return T3_E_ARG;
    t3_frames_window_plan P; t3_layout L;
    int rc = plan_frames_window(n_raw, n_frames, *cfg, fw, fh, x0, y0, w, h, out_fmt, generic_decode(), P, L); if (rc) return rc;
    if (n_frames && ((n_in && !d_in) || (P.out_bytes && !d_out))) return T3_E_ARG;
    if (n_frames > 1 && ((((uintptr_t)d_in | (uintptr_t)d_out | in_stride | out_stride) & 15u) != 0 || in_stride < P.in_stride_min || out_stride < P.out_stride_min)) return T3_E_ARG;
    Ctx& c = ctx(); if (!c.ready) return T3_E_NODEVICE;
    if (n_frames == 0 || P.out_bytes == 0) return T3_OK;
    hipStream_t s = (hipStream_t)stream;
    if (!P.one_launch || 9 * n_in >= (1ull << 32)) {        // (a stream that long: the single-frame entry's whole-frame path, frame by frame)
        for (uint32_t f = 0; f < n_frames; ++f) {
            rc = t3hip_decode_window_async((const uint8_t*)d_in + (uint64_t)f * in_stride, n_in, cfg, n_raw, fw, fh, x0, y0, w, h, (uint8_t*)d_out + (uint64_t)f * out_stride, out_fmt,
                                           d_verdict + 2 * f, stream);
            if (rc) return rc;
        }
        return T3_OK;
    }
    const t3_window_plan& wp = P.win;
    if (L.out_words > n_in) return T3_E_HEADER;                              // truncated streams (decode_body)
    const uint64_t run_stride = (6 * wp.n_px + 15u) & ~15ull;
    void* d_px; rc = scratch(c, Scratch::StreamWindow, (uint64_t)n_frames * run_stride + kWinScratchSlack, &d_px, s); if (rc) return rc;
    const ScrCycle sc = scrambler_cycle(cfg->seed_a, cfg->seed_b, cfg->seed_s0);
    // frame 0's run: the decoder addresses its output by stream pixel, so it is handed the address pixel 0 would have (t3hip_decode_window_async)
    uint8_t* const base0 = (uint8_t*)((uintptr_t)d_px - (uintptr_t)(6 * wp.first_px));
    const bool all = wp.tile_lo == 0 && wp.tile_hi == wp.n_tiles;
    // a frame's stream is its L.out_words words, whatever lies behind them in the stride (the window plan bounds 9 * out_words by 2^32)
    FusedPlan p; rc = plan_fixed_fused(9 * L.out_words, L.header_syms, L, sc, wp.first_px + wp.n_px, FusedForm::Pixels, p, 0, 0, all ? 0u : wp.tile_lo, all ? 0xFFFFFFFFu : wp.tile_hi);
    if (rc) return rc < 0 ? rc : T3_E_ARG;
    rc = launch_fused_frames(p, d_in, in_stride, base0, run_stride, n_frames, *cfg, n_raw, d_verdict, s); if (rc) return rc;
    return launch_window_crop_frames(d_px, run_stride, wp.first_px, 2 * n_raw, fw, fh, x0, y0, w, h, d_out, out_stride, out_fmt, n_frames, s);
}

// host buffers with the device strides: one upload, the device entry, one synchronisation for the verdict words, one download
int t3hip_decode_frames_window(const void* in, uint64_t n_in, uint64_t in_stride, uint32_t n_frames, const t3_cfg* cfg, uint64_t n_raw, uint32_t fw, uint32_t fh,
                               uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, void* out, uint64_t out_stride, int out_fmt, int* frame_rc) {
    if (!cfg || (n_frames && !frame_rc) || (n_frames && n_in && !in)) return T3_E_ARG;
    t3_frames_window_plan P; t3_layout L;
    int rc = plan_frames_window(n_raw, n_frames, *cfg, fw, fh, x0, y0, w, h, out_fmt, generic_decode(), P, L); if (rc) return rc;
    if (n_frames && P.out_bytes && !out) return T3_E_ARG;
    const uint64_t in_bytes = 9 * n_in;
    if (n_frames == 1) { in_stride = (in_bytes + 15u) & ~15ull; out_stride = P.out_stride_min; }
    else if (n_frames && (((in_stride | out_stride) & 15u) != 0 || in_stride < in_bytes || in_stride < P.in_stride_min || out_stride < P.out_stride_min)) return T3_E_ARG;
    Ctx& c = ctx(); if (!c.ready) return T3_E_NODEVICE;
    if (n_frames == 0) return T3_OK;
    for (uint32_t f = 0; f < n_frames; ++f) frame_rc[f] = T3_OK;
    if (P.out_bytes == 0) return T3_OK;
    std::lock_guard<std::recursive_mutex> hl(c.host_mu);
    hipStream_t s = c.stream;
    void *di, *dout;
    rc = scratch(c, Scratch::HostIn, (uint64_t)n_frames * in_stride + 64, &di); if (rc) return rc;
    const uint64_t v_off = (uint64_t)n_frames * out_stride;                               // the verdict words behind the windows
    rc = scratch(c, Scratch::HostOut, v_off + 8ull * n_frames + 64, &dout); if (rc) return rc;
    uint32_t* const d_verdict = (uint32_t*)((uint8_t*)dout + v_off);
    HIPCHK(copy_frames(di, in, in_stride, in_bytes, n_frames, hipMemcpyHostToDevice, s));
    rc = t3hip_decode_frames_window_async(di, n_in, in_stride, n_frames, cfg, n_raw, fw, fh, x0, y0, w, h, dout, out_stride, out_fmt, d_verdict, s); if (rc) return rc;
    std::vector<uint32_t> v(2 * (size_t)n_frames);
    HIPCHK(hipMemcpyAsync(v.data(), d_verdict, 8ull * n_frames, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    uint8_t want[96]; memset(want, 0, sizeof want); const int hs = header_encode(*cfg, n_raw, want);
    for (uint32_t f = 0; f < n_frames; ++f) {
        frame_rc[f] = v[2 * f + 1] ? T3_E_RS : T3_OK;
        if (!v[2 * f]) continue;
        // the header's symbols are not the expected ones: it may still decode (RS(26,18) per header block) to the caller's configuration
        // and word count -- then the frame is redone by the single-frame entry, whose block count stands -- else the frame is not of this batch
        const uint8_t* dif = (const uint8_t*)di + (uint64_t)f * in_stride;
        t3_cfg seen = *cfg; uint64_t seen_raw = 0; uint8_t next[3], got[96]; memset(got, 0, sizeof got);
        rc = read_header(dif, n_in, cfg->mode, &seen, &seen_raw, next, s);
        if (rc == T3_E_HIP || rc == T3_E_NODEVICE) return rc;
        if (rc != T3_OK || seen_raw != n_raw || header_encode(seen, seen_raw, got) != hs || memcmp(got, want, sizeof want) != 0) { frame_rc[f] = T3_E_HEADER; continue; }
        rc = t3hip_decode_window_async(dif, n_in, cfg, n_raw, fw, fh, x0, y0, w, h, (uint8_t*)dout + (uint64_t)f * out_stride, out_fmt, d_verdict + 2 * f, s);
        if (rc == T3_E_HIP || rc == T3_E_NODEVICE) return rc;
        if (rc != T3_OK) { frame_rc[f] = rc; continue; }
        uint32_t v1[2];
        HIPCHK(hipMemcpyAsync(v1, d_verdict + 2 * f, 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        frame_rc[f] = v1[1] ? T3_E_RS : T3_OK;
    }
    HIPCHK(copy_frames(out, dout, out_stride, P.out_bytes, n_frames, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return T3_OK;
}

int t3hip_decode_profile_dev(const void* d_in, uint64_t n_in, t3_cfg* seen, void* d_out, uint64_t cap, uint64_t* n_out, int to_pixels, void* stream) {
    Ctx& c = ctx(); if (!c.ready) return T3_E_NODEVICE;
    if (!seen || !n_out || (n_in && !d_in)) return T3_E_ARG;
    hipStream_t s = (hipStream_t)stream;
    *n_out = 0;
    if (seen->profile == T3_RAW_MODE) {                                       // OLD:998-1002
        const uint64_t units = to_pixels ? 2 * n_in : n_in; *n_out = units;
        if (units > cap) return T3_E_CAPACITY;
        if (!n_in) return T3_OK;
        if (to_pixels) return t3hip_unpack_words_dev(d_in, n_in, d_out, stream);
        HIPCHK(hipMemcpyAsync(d_out, d_in, n_in * 9, hipMemcpyDeviceToDevice, s));
        return T3_OK;
    }
    uint64_t n_raw = 0; uint8_t next[3];
    int rc = read_header(d_in, n_in, seen->mode, seen, &n_raw, next, s);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(c.mail_mu);
    uint32_t* const d_fail = arm_fail_mailbox(c); if (!d_fail) return T3_E_HIP;
    rc = decode_body(d_in, n_in, *seen, n_raw, next, d_out, cap, n_out, to_pixels, d_fail, s, nullptr);
    if (rc) { if (rc != T3_E_CAPACITY) *n_out = 0; return rc; }
    HIPCHK(hipStreamSynchronize(s));
    if (*(volatile uint32_t*)c.mail.fail) { *n_out = 0; return T3_E_RS; }           // OLD:987,1017: false, out stays empty
    return T3_OK;
}

// Pipelined host decode (round 3; run_chunks, as encode_host_pipelined in t3_api_encode.cpp): FIXED, one k on all bands, 1-D, no beacon, pixels
// out, a frame of many tiles.  The header is parsed on the host from the caller's buffer; the nine band runs of chunk c go up and the fused
// decoder runs on its tiles while the pixels of chunk c - 1 come down.  1: not applicable.
static int decode_host_pipelined(const void* in, uint64_t n_in, t3_cfg* seen, void* out, uint64_t cap, uint64_t* n_out, void* di, void* dout) {
    if (seen->mode != T3_MODE_FIXED || seen->profile == T3_RAW_MODE || n_in < 10 || getenv("T3HIP_SERIAL_HOST") != nullptr || generic_decode()) return 1;
    t3_cfg cfg = *seen; uint64_t n_raw = 0; uint8_t next[3];
    if (header_parse((const uint8_t*)in, n_in, T3_MODE_FIXED, cfg, &n_raw, next) != T3_OK) return 1;    // (the serial path reports it)
    t3_layout L; if (plan(n_raw, cfg, L) != T3_OK || L.out_words > n_in) return 1;
    if (L.interleave2d || L.beacon_on || 9 * n_in >= (1ull << 32) || !single_k(L)) return 1;
    const uint64_t units = 2 * n_raw;
    if (units > cap) return 1;
    const ScrCycle sc = scrambler_cycle_from_next(next, cfg.seed_s0);
    const uint32_t hs = L.header_syms, nb = fused_nb(FusedForm::Pixels);
    const uint32_t n_tiles = fused_tiles(L, FusedForm::Pixels), units_tile = fused_geom(L.band_k[0], FusedForm::Pixels).units_tile;
    const uint32_t want = host_chunks(6u);                                           // (FIXED streams start 90 symbols in: the band runs are 2-byte aligned, a strided copy of them is slow -- nine plain copies per chunk, few chunks; t3_api_encode.cpp)
    if (n_tiles < 64u) return 1;
    const uint32_t per = (n_tiles + want - 1u) / want, n_chunks = (n_tiles + per - 1u) / per;
    Ctx& c = ctx();
    *seen = cfg;                                                                       // OLD:1006-1013: the header decoded
    std::lock_guard<std::mutex> lk(c.mail_mu);
    uint32_t* const d_fail = arm_fail_mailbox(c); if (!d_fail) return T3_E_HIP;
    const bool allow_strided = getenv("T3HIP_NO_2D_COPY") == nullptr;
    uint8_t* const ho = (uint8_t*)out; const uint8_t* const dob = (const uint8_t*)dout;
    const int rc = run_chunks(c, n_chunks, [&](uint32_t ch) {
        if (ch == 0) {   // header words: the device copy of the stream starts with them (the kernel itself never reads them)
            const hipError_t er = hipMemcpyAsync(di, in, hs, hipMemcpyHostToDevice, c.stream); if (er != hipSuccess) return fail_hip(er, "hipMemcpyAsync(header)");
        }
        const uint32_t t0 = ch * per, t1 = std::min<uint32_t>(n_tiles, t0 + per);
        // (a lane's 16-byte load of a block's second half reaches 0 bytes past the block: runs are exact)
        const hipError_t er = copy_band_runs((uint8_t*)di, (const uint8_t*)in, L, hs, (uint64_t)t0 * nb, (uint64_t)t1 * nb, allow_strided, hipMemcpyHostToDevice, c.stream);
        if (er != hipSuccess) return fail_hip(er, "copy_band_runs(chunk upload)");
        FusedPlan p; int frc = plan_fixed_fused(9 * n_in, hs, L, sc, units, FusedForm::Pixels, p, 0, 0, t0, t1);
        if (frc == T3_OK) frc = bind_fused(p, dout, d_fail);
        if (frc == T3_OK) frc = launch_fixed_fused(p, (const uint8_t*)di, nullptr, c.stream);
        return frc == 1 ? T3_E_ARG : frc;
    }, [&](uint32_t ch, hipStream_t s2) {
        const uint64_t u0 = std::min<uint64_t>(units, (uint64_t)ch * per * units_tile), u1 = std::min<uint64_t>(units, ((uint64_t)ch * per + per) * units_tile);
        return u1 > u0 ? hipMemcpyAsync(ho + 6 * u0, dob + 6 * u0, 6 * (u1 - u0), hipMemcpyDeviceToHost, s2) : hipSuccess;
    });
    if (rc != T3_OK) return rc;
    *n_out = units;
    if (*(volatile uint32_t*)c.mail.fail) { *n_out = 0; return T3_E_RS; }                // OLD:987,1017
    return T3_OK;
}

static int decode_host(const void* in, uint64_t n_in, t3_cfg* seen, void* out, uint64_t cap, uint64_t* n_out, int to_pixels) {
    Ctx& c = ctx(); if (!c.ready) return T3_E_NODEVICE;
    if (!seen || !n_out || (n_in && !in)) return T3_E_ARG;
    std::lock_guard<std::recursive_mutex> hl(c.host_mu);                // one caller at a time on the shared stream and scratch
    void *di, *dout; int rc = scratch(c, Scratch::HostIn, n_in * 9 + 64, &di); if (rc) return rc;
    const uint64_t unit = to_pixels ? 6 : 9, dcap = (to_pixels ? 2 : 1) * (n_in + 16);
    rc = scratch(c, Scratch::HostOut, dcap * unit + 64, &dout); if (rc) return rc;
    hipStream_t s = c.stream;
    if (to_pixels == 1) { rc = decode_host_pipelined(in, n_in, seen, out, cap, n_out, di, dout); if (rc != 1) return rc; }   // 1: not that framing -> one upload, the kernels, one download
    if (n_in) HIPCHK(hipMemcpyAsync(di, in, n_in * 9, hipMemcpyHostToDevice, s));
    rc = t3hip_decode_profile_dev(di, n_in, seen, dout, dcap, n_out, to_pixels, s);
    if (rc) return rc;
    if (*n_out > cap) return T3_E_CAPACITY;
    if (*n_out) HIPCHK(hipMemcpyAsync(out, dout, *n_out * unit, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return T3_OK;
}
int t3hip_decode_profile(const void* in, uint64_t n_in, t3_cfg* seen, void* out, uint64_t cap, uint64_t* n_out) { return decode_host(in, n_in, seen, out, cap, n_out, 0); }
int t3hip_decode_frame(const void* in, uint64_t n_in, t3_cfg* seen, void* px, uint64_t cap_px, uint64_t* n_px) { return decode_host(in, n_in, seen, px, cap_px, n_px, 1); }

// one frame of a batch through the synchronous single-frame path (device buffers; RGB: pixels into a per-stream scratch, then the bridge)
static int decode_frame_sync(const void* di, uint64_t n_in, t3_cfg* seen, void* dout, uint64_t cap_units, int out_fmt, uint64_t* n_out, hipStream_t s) {
    if (out_fmt != 2) return t3hip_decode_profile_dev(di, n_in, seen, dout, cap_units, n_out, out_fmt, s);
    void* d_q; int rc = scratch(ctx(), Scratch::StreamRgb, 12 * (n_in + 16) + 64, &d_q, s); if (rc) return rc;
    rc = t3hip_decode_profile_dev(di, n_in, seen, d_q, 2 * (n_in + 16), n_out, 1, s); if (rc) return rc;
    if (*n_out > cap_units) return T3_E_CAPACITY;
    return t3hip_quant_to_rgb_dev(d_q, *n_out, (uint8_t*)dout, s);
}
int t3hip_decode_frames(const void* in, uint64_t n_in, uint64_t in_stride, uint32_t n_frames, void* out, uint64_t out_stride, uint64_t cap_units, int out_fmt,
                        t3_cfg* seen, uint64_t* n_out, int* frame_rc) {
    Ctx& c = ctx(); if (!c.ready) return T3_E_NODEVICE;
    if (!seen || !n_out || (n_frames && !frame_rc) || (n_frames && n_in && !in) || out_fmt < 0 || out_fmt > 2) return T3_E_ARG;
    *n_out = 0;
    if (n_frames == 0) return T3_OK;
    if (n_frames > 65535u) return T3_E_ARG;
    const uint64_t UB = out_fmt == 0 ? 9u : out_fmt == 1 ? 6u : 3u, in_bytes = 9 * n_in;
    if (n_frames == 1) { in_stride = (in_bytes + 15u) & ~15ull; out_stride = (cap_units * UB + 15u) & ~15ull; }
    else if (((in_stride | out_stride) & 15u) != 0 || in_stride < in_bytes || cap_units * UB > out_stride) return T3_E_ARG;
    if (cap_units && !out) return T3_E_ARG;
    std::lock_guard<std::recursive_mutex> hl(c.host_mu);
    hipStream_t s = c.stream;
    void *di, *dout;
    int rc = scratch(c, Scratch::HostIn, (uint64_t)n_frames * in_stride + 64, &di); if (rc) return rc;
    const uint64_t v_off = (uint64_t)n_frames * out_stride;                              // the verdict words behind the frames
    rc = scratch(c, Scratch::HostOut, v_off + 8ull * n_frames + 64, &dout); if (rc) return rc;
    uint32_t* const d_verdict = (uint32_t*)((uint8_t*)dout + v_off);
    HIPCHK(copy_frames(di, in, in_stride, in_bytes, n_frames, hipMemcpyHostToDevice, s));
    const t3_cfg seen_in = *seen;
    std::vector<uint8_t> redo(n_frames, 1);                                               // frames that take the single-frame path
    uint64_t units = 0;
    const bool batched = seen_in.profile != T3_RAW_MODE && seen_in.mode == T3_MODE_FIXED;
    bool have_units = batched;
    if (batched) {
        // frame 0's header, as t3hip_decode_profile reads it; then the batch with that configuration
        t3_cfg cfg0 = seen_in; uint64_t n_raw = 0; uint8_t next[3];
        rc = read_header(di, n_in, seen_in.mode, &cfg0, &n_raw, next, s); if (rc) return rc;
        units = out_fmt == 0 ? n_raw : 2 * n_raw;
        *n_out = units;
        if (units > cap_units) return T3_E_CAPACITY;
        rc = t3hip_decode_frames_async(di, n_in, in_stride, n_frames, &cfg0, n_raw, dout, out_stride, out_fmt, d_verdict, s); if (rc) return rc;
        std::vector<uint32_t> v(2 * (size_t)n_frames);
        HIPCHK(hipMemcpyAsync(v.data(), d_verdict, 8ull * n_frames, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        for (uint32_t f = 0; f < n_frames; ++f) { redo[f] = v[2 * f] != 0; frame_rc[f] = v[2 * f + 1] ? T3_E_RS : T3_OK; }
        *seen = cfg0;
    }
    for (uint32_t f = 0; f < n_frames; ++f) if (redo[f]) {
        t3_cfg sf = seen_in; uint64_t n = 0;
        frame_rc[f] = decode_frame_sync((const uint8_t*)di + (uint64_t)f * in_stride, n_in, &sf, (uint8_t*)dout + (uint64_t)f * out_stride, cap_units, out_fmt, &n, s);
        if (frame_rc[f] == T3_E_HIP || frame_rc[f] == T3_E_NODEVICE) return frame_rc[f];
        if (f == 0 && !batched) *seen = sf;
        if (frame_rc[f] != T3_OK) continue;
        if (!have_units) { units = n; *n_out = n; have_units = true; }
        else if (n != units) frame_rc[f] = T3_E_HEADER;                                  // a frame of another size is not of this batch
    }
    HIPCHK(copy_frames(out, dout, out_stride, units * UB, n_frames, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return T3_OK;
}

int t3hip_rs_decode_blocks_dev(int k, int mode, uint8_t* d_code, uint64_t n_blocks, uint8_t* d_data, uint8_t* d_ok, void* stream) {
    Ctx& c = ctx(); if (!c.ready) return T3_E_NODEVICE;
    if (!valid_k(k) || mode < 0 || mode > 1) return T3_E_ARG;
    if (!n_blocks) return T3_OK;
    if (!d_code || !d_data || !d_ok) return T3_E_ARG;
    hipLaunchKernelGGL(rs_decode_blocks_kernel, dim3((unsigned)((n_blocks + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_code, n_blocks, k, mode, c.d_tab, d_data, d_ok);
    HIPCHK(hipGetLastError()); return T3_OK;
}

int t3hip_inject_errors_dev(void* d_words, uint64_t first_sym, uint64_t n_blocks, uint32_t seed, int max_err, void* stream) {
    if (!ctx().ready) return T3_E_NODEVICE;
    if (max_err < 0 || max_err > 26) return T3_E_ARG;
    if (!n_blocks) return T3_OK;
    if (!d_words) return T3_E_ARG;
    hipLaunchKernelGGL(inject_errors_kernel, dim3(blocks_for(n_blocks, 1u << 20)), dim3(256), 0, (hipStream_t)stream, (uint8_t*)d_words + first_sym, n_blocks, seed, max_err);
    HIPCHK(hipGetLastError()); return T3_OK;
}

}  // extern "C"
