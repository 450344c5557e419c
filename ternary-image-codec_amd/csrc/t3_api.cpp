// t3_api.cpp — the C-ABI of libt3hip.so (include/t3hip.h): context, tile planning, kernel launches.
// Host logic only; all arithmetic on the data path happens in the kernels (t3_encode.h, t3_kernels.hip, t3_decode*.hip).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <map>
#include <mutex>
#include <string>
#include <system_error>
#include <thread>
#include <tuple>
#include <vector>

#include "../../include/t3hip.h"
#include "t3_ctx.hpp"
#include "t3_host.hpp"
#include "t3_kernels.h"
#include "t3_decode.h"

using namespace t3;

namespace {

// One context per GPU.  t3hip_init creates the process default; t3hip_create more (one per device for a host that drives a whole
// node from one process); t3hip_use binds the calling thread to one of them (thread-local), every entry point works on the
// calling thread's context: ctx().
Ctx g_null;                                               // stands in while no context exists: ready == false
Ctx* g_def = nullptr;
thread_local Ctx* tl_cur = nullptr;
}  // namespace

Ctx& t3::ctx() { return tl_cur ? *tl_cur : (g_def ? *g_def : g_null); }
int t3::fail_hip(hipError_t e, const char* what) { ctx().hip_err = std::string(what) + ": " + hipGetErrorString(e); return T3_E_HIP; }

namespace {
const int kOfIndex[4] = {24, 22, 20, 18};

// Tile-ticket counters of a persistent kernel (tile_tickets, t3_ctx.hpp): eight class counters + a done counter, 256 B apart, zero between
// launches (the kernel's last workgroup re-zeroes them).  One set per (stream, kernel kind): launches on one stream are ordered, streams are
// not.  None for hipStreamPerThread (one handle value, a different real stream per thread) or when the allocation failed.
void tile_tickets_held(Ctx& c, hipStream_t s, int kind, uint32_t grid, uint32_t** ctr, uint32_t* n_classes) {   // caller holds c.mu (the encoder's launch path does)
    constexpr uint32_t kSlots = 64, kSlotWords = 64 * 9;
    static const bool off = getenv("T3HIP_STATIC_TILES") != nullptr;      // measurement knob
    *n_classes = std::min<uint32_t>(8u, grid); *ctr = nullptr;
    if (off || s == hipStreamPerThread) return;
    if (!c.d_ctr) { if (hipMalloc((void**)&c.d_ctr, kSlots * kSlotWords * 4) != hipSuccess) { c.d_ctr = nullptr; return; } if (hipMemset(c.d_ctr, 0, kSlots * kSlotWords * 4) != hipSuccess) return; }
    const auto key = std::make_pair(s, kind);
    auto sl = c.ctr_slot.find(key);
    if (sl == c.ctr_slot.end() && c.ctr_slot.size() < kSlots) sl = c.ctr_slot.emplace(key, (uint32_t)c.ctr_slot.size()).first;
    if (sl != c.ctr_slot.end()) *ctr = c.d_ctr + kSlotWords * sl->second;
}

int grow(void*& p, size_t& cap, size_t bytes) {
    if (bytes <= cap) return T3_OK;
    if (p) HIPCHK(hipFree(p));                           // synchronises with whatever still reads it
    p = nullptr; cap = 0;
    const size_t want = bytes + bytes / 8 + 4096;
    HIPCHK(hipMalloc(&p, want));
    cap = want;
    return T3_OK;
}

int scratch_held(Ctx& c, Scratch kind, size_t bytes, void** out, hipStream_t s = nullptr) {   // caller holds c.mu
    if (kind == Scratch::HostIn || kind == Scratch::HostOut) {
        const int i = kind == Scratch::HostIn ? 0 : 1;
        const int rc = grow(c.buf[i], c.cap[i], bytes); if (rc) return rc;
        *out = c.buf[i];
        return T3_OK;
    }
    static thread_local char per_thread_key;              // hipStreamPerThread is one handle value but a different stream in every thread
    if (s == hipStreamPerThread) s = (hipStream_t)(void*)&per_thread_key;
    auto& e = c.sbuf[std::make_pair(kind, s)];
    const int rc = grow(e.first, e.second, bytes); if (rc) return rc;
    *out = e.first;
    return T3_OK;
}

int get_lut(Ctx& c, uint32_t kmask, int mode, const LutImage** out) {
    const uint32_t key = kmask | (uint32_t)mode << 8;
    auto it = c.luts.find(key);
    if (it == c.luts.end()) {
        LutImage L; std::vector<uint32_t> all;
        for (int i = 0; i < 4; ++i) if (kmask >> i & 1) {
            std::vector<uint32_t> img; build_encode_lut(kOfIndex[i], mode, img);
            L.k_off[i] = (uint32_t)all.size() * 4u;
            all.insert(all.end(), img.begin(), img.end());
        }
        L.bytes = (uint32_t)all.size() * 4u;
        HIPCHK(hipMalloc((void**)&L.d_img, L.bytes ? L.bytes : 16));
        HIPCHK(hipMemcpy(L.d_img, all.data(), L.bytes, hipMemcpyHostToDevice));
        it = c.luts.emplace(key, L).first;
    }
    *out = &it->second;
    return T3_OK;
}

// tables of the matrix-core encoder for one k (single-k launches)
int get_mfma_lut(Ctx& c, int k, int mode, const LutImage** out) {
    const uint32_t key = 1u << k_index(k) | (uint32_t)mode << 8 | 1u << 16;
    auto it = c.luts.find(key);
    if (it == c.luts.end()) {
        LutImage L; std::vector<uint32_t> afrag, img; build_mfma_encode(k, mode, afrag, img);
        L.bytes = (uint32_t)img.size() * 4u;
        HIPCHK(hipMalloc((void**)&L.d_img, L.bytes)); HIPCHK(hipMemcpy(L.d_img, img.data(), L.bytes, hipMemcpyHostToDevice));
        HIPCHK(hipMalloc((void**)&L.d_afrag, afrag.size() * 4)); HIPCHK(hipMemcpy(L.d_afrag, afrag.data(), afrag.size() * 4, hipMemcpyHostToDevice));
        it = c.luts.emplace(key, L).first;
    }
    *out = &it->second;
    return T3_OK;
}

// tables of the UEP matrix-core kernel: the k-independent T/M image, then the A operand of every k in use (k_off = its offset)
int get_mfma_group_lut(Ctx& c, uint32_t kmask, int mode, const LutImage** out) {
    const uint32_t key = kmask | (uint32_t)mode << 8 | 2u << 16;
    auto it = c.luts.find(key);
    if (it == c.luts.end()) {
        LutImage L; std::vector<uint32_t> all;
        for (int i = 0; i < 4; ++i) if (kmask >> i & 1) {
            std::vector<uint32_t> afrag, img; build_mfma_encode(kOfIndex[i], mode, afrag, img);
            if (all.empty()) all = img;                                   // T and M tables do not depend on k
            L.k_off[i] = (uint32_t)all.size() * 4u;
            all.insert(all.end(), afrag.begin(), afrag.end());
        }
        L.bytes = (uint32_t)all.size() * 4u;
        HIPCHK(hipMalloc((void**)&L.d_img, L.bytes)); HIPCHK(hipMemcpy(L.d_img, all.data(), L.bytes, hipMemcpyHostToDevice));
        it = c.luts.emplace(key, L).first;
    }
    *out = &it->second;
    return T3_OK;
}

uint32_t round16(uint32_t x) { return (x + 15u) & ~15u; }

// ------------------------------------------------------------------------------------------------
// K2 launch planning: one launch covers a set of bands whose k's have a manageable lcm
// ------------------------------------------------------------------------------------------------
enum class EncKind { MfmaK, Uep, Lut };     // matrix cores: one k on all nine bands / bands grouped by k (UEP); LUT fallback
// One K2 launch.  Its arguments lack only what depends on the stream: the tile tickets, and body_out when the beacon pass follows.
struct EncLaunch { EncArgs a; const void* fn; uint32_t block; EncKind kind; };
struct EncPlan { EncLaunch l[2]; uint32_t n = 0; bool beacon_pass = false; BeaconArgs b; };   // a frame's launches, then the beacon pass

// Phase 1 (pixels) gives a lane four consecutive pixel triples: waves that cover the worst-placed tile of TS symbols
// (tile starts cycle through S0 mod 52)
uint32_t p1_waves_per_parity(uint32_t TS) {
    uint32_t worst = 0;
    for (uint32_t t = 0; t < 52; ++t) {
        const uint64_t S0 = (uint64_t)t * TS;
        const uint64_t t_base = (S0 / 13) & ~3ull, t_end = (S0 + TS + 12) / 13;
        worst = std::max<uint32_t>(worst, (uint32_t)((t_end - t_base + 3) / 4));
    }
    return (worst + 63) / 64;
}

// ... and for raw words (1-D): four word triples = 104 symbols per lane (convert_words_packed)
uint32_t p1_waves_words(uint32_t TS) {
    uint32_t worst = 0;
    for (uint32_t t = 0; t < 104; ++t) {
        const uint64_t S0 = (uint64_t)t * TS;
        const uint64_t t_base = (S0 / 26) & ~3ull, t_end = (S0 + TS + 25) / 26;
        worst = std::max<uint32_t>(worst, (uint32_t)((t_end - t_base + 3) / 4));
    }
    return (worst + 63) / 64;
}

// One launch of `kind` over the bands of band_mask (lut: its tables): tile, LDS carve-up, arguments; false when no tile fits.  UEP on
// the matrix cores: bands are grouped by k, a group's blocks of a tile are dealt linearly into sets of 32; eight waves take two sets each
bool plan_enc_group(const t3_layout& L, const t3_cfg& cfg, uint32_t band_mask, int fe, const LutImage& lut, EncKind kind, EncLaunch& out) {
    EncArgs& a = out.a; memset(&a, 0, sizeof a);
    const bool grp = kind == EncKind::Uep;
    const bool il2d = L.interleave2d && cfg.tile_w > 1;                  // rows of one symbol: the boustrophedon map is the identity (and the kernels' row divisions assume >= 2)
    const uint32_t GS = fe_px(fe) ? kGroupSyms : kGroupSymsW, GB = fe == FE_PIXELS ? kGroupBytes : fe == FE_RGB ? kGroupBytesRgb : kGroupBytesW;
    uint64_t Lk = 2;
    for (int b = 0; b < 9; ++b) if (band_mask >> b & 1) Lk = lcm64(Lk, L.band_k[b]);
    uint32_t lut_bytes = lut.bytes;
    // 2-D through the pipelined flow (pixel / RGB input): rows up to 512 symbols -- a tile's input covers the row segments it overlaps (up to
    // w - 1 extra symbols each side) and a permutation pass follows phase 1 (il_async 1); wider rows -- the tile's pre-interleave symbols
    // are up to three runs, staged one behind the other at 1-KiB pitches, and phase 1 stores each symbol at its post-interleave place
    // (il_async 2; t3_enc_convert.h, il_runs)
    const uint32_t il_async = !(il2d && fe_px(fe)) ? 0u : cfg.tile_w <= 512 ? 1u : 2u;
    const uint32_t il_extra = il_async == 1u ? 2u * cfg.tile_w : 0u;
    const uint32_t il_stage = il_async == 2u ? 2u * (1024u + 4u * GB + 32u) : 0u;   // two more runs: their rounding and pitch
    const uint32_t hdr = grp ? (uint32_t)kLdsHdrUep : (uint32_t)kLdsHdr;
    const bool words_packed = fe == FE_WORDS && !il2d;                     // 1-D raw words: the packed converter (whole lanes of 104 symbols: wider slack)
    const uint32_t sym_front = words_packed ? (uint32_t)kSymSlackW : (uint32_t)kSymFront, sym_back = words_packed ? (uint32_t)kSymSlackW : (uint32_t)kSymBack;
    bool mixed = false;
    { int k0 = 0; for (int b = 0; b < 9; ++b) if (band_mask >> b & 1) { if (!k0) k0 = L.band_k[b]; else if (k0 != L.band_k[b]) mixed = true; } }
    // pick q: tile = 9*Lk*q stream symbols; band b then owns Lk*q/k_b blocks
    double best_score = -1; uint32_t best_q = 0;
    for (int pass = 0; pass < 2 && !best_q; ++pass) {
        const uint32_t budget = pass == 0 ? kLdsThreeWgs : 160u * 1024u;
        for (uint32_t q = 1; q <= 4096; ++q) {
            if (mixed && !grp && (q & 1u)) continue;                     // mixed k, LUT kernel: even multipliers only (measured: odd ones halve its speed)
            const uint64_t Lq = Lk * q; if (9 * Lq > 60000) break;
            uint32_t waves = 0, blocks_total = 0;
            for (int b = 0; b < 9; ++b) if (band_mask >> b & 1) {
                const uint32_t nb = (uint32_t)(Lq / L.band_k[b]);
                blocks_total += nb;
            }
            waves = (blocks_total + 63) / 64;                          // lanes are dealt to blocks linearly across bands
            uint32_t sets = 0;
            if (grp) {
                for (int i = 0; i < 4; ++i) { uint32_t items = 0; for (int b = 0; b < 9; ++b) if ((band_mask >> b & 1) && k_index(L.band_k[b]) == i) items += (uint32_t)(Lq / L.band_k[b]); sets += (items + 31) / 32; }
                if (sets > (uint32_t)kMaxSets || pass > 0) break;
                waves = 8;
            }
            if (waves > (pass == 0 ? 8u : (uint32_t)kMaxWaves)) break;   // pass 0: 512-thread workgroups, three per CU
            const uint32_t groups = (uint32_t)((9 * Lq + il_extra) / GS) + 8;
            uint32_t stage = groups * GB + 1024 + 32 + il_stage;                                              // +1 KiB: LDS-DMA pieces are whole
            if (il_async == 1u) stage = std::max<uint32_t>(stage, (uint32_t)(9 * Lq) + 64u);                  // the permutation pass writes the tile's 9 Lq symbols into the consumed stage buffer (RGB input is smaller than that)
            const uint32_t total = hdr + round16(lut_bytes) + sym_front + round16((uint32_t)(9 * Lq) + il_extra) + sym_back + ((il2d && !il_async) ? 1u : 2u) * round16(stage) + (fe == FE_RGB ? 256u : 0u);
            if (total > budget) break;
            // wave-instructions per stream symbol: phase 2 costs ~180 per wave, phase 1 (pixels) ~120 per wave-iteration
            const uint32_t wpp = words_packed ? p1_waves_words((uint32_t)(9 * Lq)) : p1_waves_per_parity((uint32_t)(9 * Lq) + il_extra + (il_async == 2u ? 312u : 0u));   // (three runs: up to six lane units of rounding)
            if ((fe_px(fe) || words_packed) && (words_packed ? 2u : 1u) * wpp > std::max(waves, 4u)) continue;
            // UEP kernel: the phases are barrier-separated and a wave runs its sets one after the other, so a tile costs one
            // phase-1 pass plus ceil(sets / 8) set times, whatever the number of busy waves
            // + a fixed cost per tile (barriers, ticket, prefetch issue, the runs' rounding in 2-D): without it the model preferred tiles of
            // 5 full waves to larger ones of 7-8 partly filled waves, measured 2-12 % slower (profiles/r03/notes.md: tile sweeps)
            const double cost = grp ? (220.0 + 100.0 * ((sets + 7) / 8)) / (double)(9 * Lq)
                                    : (600.0 + 180.0 * waves + (fe_px(fe) ? 220.0 * wpp : words_packed ? 250.0 * wpp : 180.0 * waves)) / (double)(9 * Lq);
            const double score = 1.0 / cost + 1e-9 * (double)Lq;
            if (score > best_score) { best_score = score; best_q = q; }
        }
    }
    if (!best_q) return false;
    const uint32_t Lq = (uint32_t)(Lk * best_q);
    a.Lq = Lq; a.lut_bytes = round16(lut_bytes);
    uint32_t off = hdr + a.lut_bytes;
    off += sym_front; a.sym_off = off; off += round16(9 * Lq + il_extra) + sym_back;   // slack either side: phase 1 writes whole pixel triples / whole lanes of word triples
    a.stage_off = off;
    a.stage_groups = (9 * Lq + il_extra) / GS + 8;
    uint32_t nw = 0, n_tiles = 0;
    fill_bands(a, L);
    for (int b = 0; b < 9; ++b) {
        a.band_k[b] = L.band_k[b];
        a.band_lut_off[b] = hdr + lut.k_off[k_index(L.band_k[b])];
        if (!(band_mask >> b & 1)) { a.band_nb_tile[b] = 0; a.band_blocks[b] = 0; continue; }
        const uint32_t nb = Lq / L.band_k[b];
        a.band_nb_tile[b] = nb;
        nw += nb;
        n_tiles = std::max<uint32_t>(n_tiles, (uint32_t)((L.band_blocks[b] + nb - 1) / nb));
    }
    a.n_items = nw; a.n_tiles = n_tiles;
    { uint32_t acc = 0; for (int b = 0; b < 9; ++b) { a.band_first[b] = acc; acc += a.band_nb_tile[b]; } a.band_first[9] = acc; }
    a.stage_stride = round16(std::max<uint32_t>(a.stage_groups * GB + 1024 + 32 + il_stage, il_async == 1u ? 9u * Lq + 64u : 0u));
    a.lds_bytes = a.stage_off + ((il2d && !il_async) ? 1u : 2u) * a.stage_stride;   // pipelined flow: two stage buffers (the next tile streams in early)
    if (fe == FE_RGB) { a.qt_off = a.lds_bytes; a.lds_bytes += 256u; }                            // chroma quantiser table of the fused bridge
    a.il_async = il_async;
    a.n_sym = (uint32_t)L.n_sym;
    const ScrCycle sc = scrambler_cycle(cfg.seed_a, cfg.seed_b, cfg.seed_s0);
    a.cyc24 = sc.cyc24; a.pre0 = sc.pre[0]; a.pre1 = sc.pre[1];
    mfma_scrambler_table(L.band_k[0], sc, a.scr);
    a.il_on = il2d;
    if (a.il_on) {
        const uint64_t A = (uint64_t)cfg.tile_w * cfg.tile_h;
        a.il_w = cfg.tile_w; a.il_A = (uint32_t)std::min<uint64_t>(A, std::max<uint64_t>(L.n_sym, 1));
        a.div_A = to_dev(fastdiv(a.il_A)); a.div_w = to_dev(fastdiv(a.il_w));
    }
    out.kind = kind; out.block = grp ? 512u : 64u * std::max<uint32_t>((nw + 63) / 64, 4u);
    a.p1_wpp = words_packed ? p1_waves_words(9 * Lq) : p1_waves_per_parity(9 * Lq + il_extra + (il_async == 2u ? 312u : 0u));
    a.nb_uniform = !mixed && band_mask == 0x1FF ? a.band_nb_tile[0] : 0u; a.div_nb = to_dev(fastdiv(a.nb_uniform ? a.nb_uniform : 1u));
    if (grp) {
        uint32_t ng = 0, ns = 0;
        for (int i = 0; i < 4; ++i) {
            EncArgs::Grp& G = a.grp[ng]; memset(&G, 0, sizeof G);
            uint32_t nbands = 0;
            for (int b = 0; b < 9; ++b) if ((band_mask >> b & 1) && k_index(L.band_k[b]) == i) G.bands[nbands++] = (uint8_t)b;
            if (!nbands) continue;
            G.nb = Lq / (uint32_t)kOfIndex[i]; G.div_nb = to_dev(fastdiv(G.nb)); G.n_items = nbands * G.nb; G.r = 26u - (uint32_t)kOfIndex[i];
            G.afrag_off = hdr + lut.k_off[i];
            mfma_scrambler_table(kOfIndex[i], sc, G.scr);
            for (uint32_t it0 = 0; it0 < G.n_items; it0 += 32) a.set_tab[ns++] = ng | it0 << 8;
            ++ng;
        }
        a.n_grp = ng; a.n_sets = ns;
    }
    return true;
}

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
bool equal_band_runs(const t3_layout& L) {                // the nine bands equally long, their pitch 4-byte aligned (copy_band_runs)
    for (int b = 1; b < 9; ++b) if (L.band_blocks[b] != L.band_blocks[0]) return false;
    return (26 * L.band_blocks[0]) % 4u == 0;
}

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
        if (!plan_enc_group(L, cfg, 0x1FF, fe, *lut, EncKind::Lut, probe)) {
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
        if (!plan_enc_group(L, cfg, m, fe, *lut, one_k ? EncKind::MfmaK : EncKind::Uep, e) || e.block > 512) {
            rc = get_lut(c, km, cfg.mode, &lut); if (rc) return rc;
            if (!plan_enc_group(L, cfg, m, fe, *lut, EncKind::Lut, e)) return T3_E_ARG;
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

extern "C" {

int t3hip_device_count(void) { int n = 0; if (hipGetDeviceCount(&n) != hipSuccess) return 0; return n; }

static int ctx_init_in(Ctx* c, int device);
static void ctx_teardown(Ctx* c);
// Builds `c` on `device`.  The calling thread's current context is `c` for the whole of it, so a HIP error (HIPCHK) is recorded in `c` (and
// copied to the null context for t3hip_last_hip_error after a failed create); what a failed build had already allocated is released.
static int ctx_init(Ctx* c, int device) {
    Ctx* const prev = tl_cur; tl_cur = c;
    const int rc = ctx_init_in(c, device);
    tl_cur = prev;
    if (rc) { const std::string err = c->hip_err; ctx_teardown(c); g_null.hip_err = err; c->hip_err = err; }
    return rc;
}
static int ctx_init_in(Ctx* c, int device) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n) return T3_E_NODEVICE;
    HIPCHK(hipSetDevice(device));
    hipDeviceProp_t p; HIPCHK(hipGetDeviceProperties(&p, device));
    if (std::string(p.gcnArchName).find("gfx950") == std::string::npos) { c->hip_err = std::string("not a gfx950 device: ") + p.gcnArchName; return T3_E_NODEVICE; }
    c->n_cu = p.multiProcessorCount > 0 ? p.multiProcessorCount : 256;
    HIPCHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    const Field& F = field();
    HIPCHK(hipMalloc((void**)&c->d_tab, sizeof(RsTables)));
    HIPCHK(hipMemcpy(c->d_tab, &F.t, sizeof(RsTables), hipMemcpyHostToDevice));
    for (int i = 0; i < 4; ++i) for (int m = 0; m < 2; ++m) {
        uint8_t P[24 * 8]; rs_parity_matrix(kOfIndex[i], m, P);
        HIPCHK(hipMalloc((void**)&c->d_P[i][m], sizeof P));
        HIPCHK(hipMemcpy(c->d_P[i][m], P, sizeof P, hipMemcpyHostToDevice));
    }
    HIPCHK(hipMalloc((void**)&c->d_flag, 64));
    c->dev = device;
    int rc = decode_init(c->dec);
    if (!rc) rc = crc_init(*c);
    if (rc) return rc;
    c->ready = true;
    return T3_OK;
}
// Frees everything `c` holds, also of a partly built context (ctx_init failed): every member is null-safe.  No other thread uses `c` by
// then.  The calling thread's current context is left alone, unless it is `c`.
static void ctx_teardown(Ctx* c) {
    if (c->dev >= 0) { (void)hipSetDevice(c->dev); (void)hipDeviceSynchronize(); }
    for (auto& kv : c->luts) { free_dev(kv.second.d_img); free_dev(kv.second.d_afrag); }
    c->luts.clear();
    for (auto& kv : c->sbuf) free_dev(kv.second.first);
    c->sbuf.clear();
    for (int i = 0; i < 2; ++i) { free_dev(c->buf[i]); c->cap[i] = 0; }
    for (auto& P : c->d_P) for (uint8_t*& p : P) free_dev(p);
    c->dec.release(); c->crc.release(); c->rgb.release(); c->mail.release();
    free_dev(c->d_ctr); c->ctr_slot.clear();
    for (hipEvent_t e : c->chunk_ev) (void)hipEventDestroy(e);
    c->chunk_ev.clear();
    if (c->stream2) { (void)hipStreamDestroy(c->stream2); c->stream2 = nullptr; }
    free_dev(c->d_tab); free_dev(c->d_flag);
    if (c->stream) { (void)hipStreamDestroy(c->stream); c->stream = nullptr; }
    c->ready = false; c->dev = -1;
    if (tl_cur == c) tl_cur = nullptr;
}
static std::mutex g_ctx_mu;

int t3hip_init(int device) {
    std::lock_guard<std::mutex> lk(g_ctx_mu);
    if (g_def && g_def->ready) return g_def->dev == device ? T3_OK : T3_E_ARG;      // the default context stays on its device: t3hip_shutdown first, or t3hip_create
    if (!g_def) g_def = new Ctx();
    const int rc = ctx_init(g_def, device);
    if (rc) { delete g_def; g_def = nullptr; }
    return rc;
}

int t3hip_shutdown(void) {
    std::lock_guard<std::mutex> lk(g_ctx_mu);
    if (!g_def) return T3_OK;
    if (g_def->ready) ctx_teardown(g_def);
    if (tl_cur == g_def) tl_cur = nullptr;
    delete g_def; g_def = nullptr;
    return T3_OK;
}

int t3hip_create(int device, t3hip_ctx** out) {
    if (!out) return T3_E_ARG;
    std::lock_guard<std::mutex> lk(g_ctx_mu);
    int prev_dev = -1; (void)hipGetDevice(&prev_dev);
    Ctx* c = new Ctx();
    const int rc = ctx_init(c, device);
    if (prev_dev >= 0) (void)hipSetDevice(prev_dev);
    if (rc) { delete c; return rc; }
    *out = (t3hip_ctx*)c;
    return T3_OK;
}
int t3hip_destroy(t3hip_ctx* h) {
    if (!h) return T3_OK;
    std::lock_guard<std::mutex> lk(g_ctx_mu);
    Ctx* c = (Ctx*)h;
    if (c == g_def) return T3_E_ARG;                      // the default context goes with t3hip_shutdown
    int prev_dev = -1; (void)hipGetDevice(&prev_dev);
    if (c->ready) ctx_teardown(c);
    if (tl_cur == c) tl_cur = nullptr;
    if (prev_dev >= 0) (void)hipSetDevice(prev_dev);
    delete c;
    return T3_OK;
}
int t3hip_use(t3hip_ctx* h) {
    Ctx* c = (Ctx*)h;
    if (c && !c->ready) return T3_E_ARG;
    tl_cur = c;
    Ctx& eff = ctx();                                     // c, or the default context when c is null
    if (eff.ready) HIPCHK(hipSetDevice(eff.dev));
    return T3_OK;
}
t3hip_ctx* t3hip_current(void) { Ctx& c = ctx(); return c.ready ? (t3hip_ctx*)&c : nullptr; }
int t3hip_ctx_device(const t3hip_ctx* h) { const Ctx* c = h ? (const Ctx*)h : &ctx(); return c->ready ? c->dev : -1; }
int t3hip_is_ready(void) { return ctx().ready ? 1 : 0; }
const char* t3hip_strerror(int c) {
    switch (c) {
        case T3_OK: return "ok"; case T3_E_NODEVICE: return "no usable gfx950 device (t3hip_init not done or failed)";
        case T3_E_HIP: return "HIP runtime error"; case T3_E_ARG: return "bad argument"; case T3_E_CAPACITY: return "output buffer too small";
        case T3_E_HEADER: return "superframe header did not decode (RS/CRC-12)"; case T3_E_RS: return "uncorrectable RS block";
        case T3_E_COMM: return "RCCL unavailable or collective failed";
    }
    return "unknown";
}
const char* t3hip_last_hip_error(void) { return ctx().hip_err.c_str(); }
const char* t3hip_version(void) { return "t3hip 0.1 (gfx950)"; }

// ---- host-only metadata ---------------------------------------------------------------------------------
void t3hip_cfg_default(t3_cfg* c) {
    memset(c, 0, sizeof *c);
    c->profile = T3_P2_RS26_22; for (int b = 0; b < 9; ++b) c->band_profile[b] = 1;     // OLD:864,898
    c->seed_a = c->seed_b = c->seed_s0 = 1; c->superframe_words = 8192; c->subword = 27; c->centered = 1;
}
int t3hip_plan(uint64_t n_raw, const t3_cfg* cfg, t3_layout* out) { if (!cfg || !out) return T3_E_ARG; return plan(n_raw, *cfg, *out); }
uint64_t t3hip_encoded_words(uint64_t n_raw, const t3_cfg* cfg) { t3_layout L; if (!cfg || plan(n_raw, *cfg, L) != T3_OK) return 0; return L.out_words; }
int t3hip_gf27_tables(uint8_t* e78, int16_t* l27, uint8_t* m729, uint8_t* i27) {
    const Field& F = field();
    if (e78) memcpy(e78, F.exp78, 78); if (l27) memcpy(l27, F.log, sizeof F.log);
    if (m729) memcpy(m729, F.t.mul, 729); if (i27) memcpy(i27, F.t.inv, 27);
    return T3_OK;
}
int t3hip_rs_generator(int k, uint8_t* g_out) { if (!valid_k(k) || !g_out) return T3_E_ARG; rs_generator(k, g_out); return T3_OK; }
int t3hip_mfma_encode_tables(int k, int mode, uint32_t* afrag, uint32_t* lds_img) {
    if (!valid_k(k) || !afrag || !lds_img || mode < 0 || mode > 1) return T3_E_ARG;
    std::vector<uint32_t> a, l; build_mfma_encode(k, mode, a, l);
    memcpy(afrag, a.data(), a.size() * 4); memcpy(lds_img, l.data(), l.size() * 4);
    return T3_OK;
}
int t3hip_rs_parity_matrix(int k, int mode, uint8_t* P) { if (!valid_k(k) || !P || mode < 0 || mode > 1) return T3_E_ARG; rs_parity_matrix(k, mode, P); return T3_OK; }
int t3hip_header_pack(const t3_cfg* c, uint32_t fs, uint32_t bh, uint8_t s[27]) { if (!c || !s) return T3_E_ARG; header_pack(*c, fs, bh, s); return T3_OK; }
int t3hip_header_check(const uint8_t s[27]) { return s && header_check(s) ? 1 : 0; }
int t3hip_header_unpack(const uint8_t s[27], t3_cfg* o, uint32_t* fs, uint32_t* bh) { if (!s || !o) return T3_E_ARG; header_unpack(s, *o, fs, bh); return T3_OK; }
int t3hip_header_encode(const t3_cfg* c, uint64_t n_raw, uint8_t* out, uint32_t* n) {
    if (!c || !out || !n) return T3_E_ARG;
    t3_layout L; int rc = plan(n_raw, *c, L); if (rc) return rc;
    if (c->profile == T3_RAW_MODE) { *n = 0; return T3_OK; }
    *n = (uint32_t)header_encode(*c, n_raw, out); return T3_OK;
}

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
    { std::lock_guard<std::mutex> lk(c.mu); rc = scratch_held(c, Scratch::HostIn, n_units * (fe == FE_PIXELS ? 6 : 9) + 64, &di); if (rc) return rc; rc = scratch_held(c, Scratch::HostOut, L.out_words * 9 + 64, &dout); if (rc) return rc; }
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

// ---- timing helper ------------------------------------------------------------------------------------------
// Timing only: a plain hipEventCreate event ends every record in a system-scope release (cache write-back and invalidate, ~4 us of
// stream time, and the kernel behind it starts cold).  These events order nothing and publish nothing, so they are created without
// that fence (profiles/launch_fixed_costs/notes.md).  T3_EVENT_FLAGS: measurement builds only.
#ifndef T3_EVENT_FLAGS
#define T3_EVENT_FLAGS hipEventDisableSystemFence
#endif
int t3hip_event_create(void** ev) { if (!ctx().ready) return T3_E_NODEVICE; hipEvent_t e; HIPCHK(hipEventCreateWithFlags(&e, T3_EVENT_FLAGS)); *ev = e; return T3_OK; }
int t3hip_event_record(void* ev, void* stream) { HIPCHK(hipEventRecord((hipEvent_t)ev, (hipStream_t)stream)); return T3_OK; }
int t3hip_event_elapsed_ms(void* a, void* b, float* ms) { HIPCHK(hipEventSynchronize((hipEvent_t)b)); HIPCHK(hipEventElapsedTime(ms, (hipEvent_t)a, (hipEvent_t)b)); return T3_OK; }
int t3hip_event_destroy(void* ev) { HIPCHK(hipEventDestroy((hipEvent_t)ev)); return T3_OK; }

}  // extern "C"

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
        const uint64_t maxb = *std::max_element(L.band_blocks, L.band_blocks + 9);
        tiles = (uint32_t)((maxb + (uint32_t)T3_DEC_PX_NB - 1) / (uint32_t)T3_DEC_PX_NB);
    } else {
        LutImage lut; lut.bytes = (uint32_t)kMfmaLdsBytes;                       // the tile depends on the tables' size alone: no device
        EncLaunch e;
        if (!plan_enc_group(L, cfg, 0x1FF, fe_of_fmt(fmt), lut, EncKind::MfmaK, e) || e.block > 512u) return T3_OK;
        tiles = e.a.n_tiles;
    }
    if (tiles == 0) return T3_OK;
    if ((uint64_t)n_frames * tiles >= (1ull << 31)) return T3_E_ARG;
    out.tiles_per_frame = tiles; out.one_launch = 1;
    return T3_OK;
}
int encode_rgb_fused(const void* d_rgb, uint64_t n_px, const t3_cfg* cfg, void* d_out, uint64_t cap, uint64_t* n_out, hipStream_t s) { return encode_dev(FE_RGB, d_rgb, n_px, cfg, d_out, cap, n_out, s); }
int scratch(Ctx& c, Scratch kind, size_t bytes, void** out, hipStream_t s) { std::lock_guard<std::mutex> lk(c.mu); return scratch_held(c, kind, bytes, out, s); }
void tile_tickets(Ctx& c, hipStream_t s, int kind, uint32_t grid, uint32_t** ctr, uint32_t* n_classes) { std::lock_guard<std::mutex> lk(c.mu); tile_tickets_held(c, s, kind, grid, ctr, n_classes); }
int resident_grid(Ctx& c, const void* fn, int threads, uint32_t lds_bytes, uint64_t n_items, bool round_lds_units, uint32_t* grid) {
    static std::map<std::tuple<const void*, int, int, uint32_t>, int> occ; static std::mutex occ_mu;   // per device: the attribute is set on the device's copy of the function
    int per_cu;
    {
        std::lock_guard<std::mutex> lk(occ_mu);
        const auto key = std::make_tuple(fn, c.dev, threads, lds_bytes);
        auto it = occ.find(key);
        if (it == occ.end()) {
            HIPCHK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
            int o = 1; HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&o, fn, threads, lds_bytes));
            it = occ.emplace(key, o).first;
        }
        per_cu = it->second;
    }
    if (round_lds_units) per_cu = std::min<int>(per_cu, (int)(kLdsUnitsPerCu / ((lds_bytes + kLdsUnit - 1u) / kLdsUnit)));
    *grid = (uint32_t)std::max<uint64_t>(1u, std::min<uint64_t>(n_items, (uint64_t)c.n_cu * (uint64_t)std::max(1, per_cu)));
    return T3_OK;
}
hipError_t copy_band_runs(uint8_t* dst, const uint8_t* src, const t3_layout& L, uint32_t hs, uint64_t blk_lo, uint64_t blk_hi,
                          bool allow_strided, hipMemcpyKind kind, hipStream_t s) {
    // every copy costs ~20 us of the issuing thread; a strided copy at 2-byte alignment falls off a cliff (encode_host_pipelined)
    const uint64_t off = hs + L.band_body_off[0] + 26 * blk_lo, width = 26 * (blk_hi - blk_lo), pitch = 26 * L.band_blocks[0];
    if (allow_strided && equal_band_runs(L) && blk_hi <= L.band_blocks[0] && off % 4u == 0 && width % 4u == 0)
        return hipMemcpy2DAsync(dst + off, pitch, src + off, pitch, width, 9, kind, s);
    for (int b = 0; b < 9; ++b) {
        const uint64_t lo = std::min<uint64_t>(L.band_blocks[b], blk_lo), hi = std::min<uint64_t>(L.band_blocks[b], blk_hi), o = hs + L.band_body_off[b] + 26 * lo;
        if (hi > lo) { const hipError_t er = hipMemcpyAsync(dst + o, src + o, 26 * (hi - lo), kind, s); if (er != hipSuccess) return er; }
    }
    return hipSuccess;
}
uint32_t host_chunks(uint32_t dflt) { static const uint32_t env = getenv("T3HIP_HOST_CHUNKS") ? (uint32_t)atoi(getenv("T3HIP_HOST_CHUNKS")) : 0u; return env ? env : dflt; }
int run_chunks(Ctx& c, uint32_t n_chunks, const std::function<int(uint32_t ch)>& upload_and_launch,
               const std::function<hipError_t(uint32_t ch, hipStream_t s2)>& download) {
    if (!c.stream2) HIPCHK(hipStreamCreateWithFlags(&c.stream2, hipStreamNonBlocking));
    while (c.chunk_ev.size() < n_chunks) { hipEvent_t ev; HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming)); c.chunk_ev.push_back(ev); }
    const hipStream_t s2 = c.stream2; const hipEvent_t* const evs = c.chunk_ev.data(); const int dev = c.dev;
    std::atomic<uint32_t> launched{0}; std::atomic<int> abort_dl{0};
    hipError_t dl_err = hipSuccess; int rc = T3_OK;
    try {
        std::thread dl([&] {                                // chunk ch's download, once its event has fired
            if (hipSetDevice(dev) != hipSuccess) { dl_err = hipErrorInvalidDevice; return; }
            for (uint32_t ch = 0; ch < n_chunks; ++ch) {
                while (launched.load(std::memory_order_acquire) <= ch) { if (abort_dl.load()) return; std::this_thread::yield(); }
                hipError_t er = hipEventSynchronize(evs[ch]);
                if (er == hipSuccess) er = download(ch, s2);
                if (er != hipSuccess) { dl_err = er; return; }
            }
            dl_err = hipStreamSynchronize(s2);
        });
        for (uint32_t ch = 0; ch < n_chunks && rc == T3_OK; ++ch) {
            rc = upload_and_launch(ch);
            if (rc == T3_OK) { const hipError_t er = hipEventRecord(evs[ch], c.stream); if (er != hipSuccess) rc = fail_hip(er, "hipEventRecord"); }
            if (rc == T3_OK) launched.store(ch + 1, std::memory_order_release);
        }
        if (rc != T3_OK) abort_dl.store(1);
        dl.join();
    } catch (const std::system_error&) {                    // only from the thread's constructor (past it, unwinding would meet a joinable
        return 1;                                           // thread and terminate): nothing issued yet
    }
    if (rc == T3_OK && dl_err != hipSuccess) rc = fail_hip(dl_err, "run_chunks: chunk download");
    if (rc == T3_OK) HIPCHK(hipStreamSynchronize(c.stream));
    else { (void)hipStreamSynchronize(s2); (void)hipStreamSynchronize(c.stream); }   // nothing left in flight into the caller's buffers
    return rc;
}
int host_stage(Ctx& c, const void* in, uint64_t in_bytes, void** di, uint64_t out_bytes, void** dout) {
    int rc = scratch(c, Scratch::HostIn, in_bytes + 64, di); if (rc) return rc;
    rc = scratch(c, Scratch::HostOut, out_bytes + 64, dout); if (rc) return rc;
    if (in_bytes) HIPCHK(hipMemcpyAsync(*di, in, in_bytes, hipMemcpyHostToDevice, c.stream));
    return T3_OK;
}
int host_fetch(Ctx& c, void* out, const void* dout, uint64_t bytes) {
    if (bytes) HIPCHK(hipMemcpyAsync(out, dout, bytes, hipMemcpyDeviceToHost, c.stream));
    HIPCHK(hipStreamSynchronize(c.stream)); return T3_OK;
}
}  // namespace t3
