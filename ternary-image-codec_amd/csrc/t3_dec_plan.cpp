// t3_dec_plan.cpp — the decode side's planner (t3_dec_plan.hpp).  Host arithmetic only.
#include "t3_dec_plan.hpp"

#include <string.h>

namespace t3 {
namespace {
uint32_t round16(uint32_t x) { return (x + 15u) & ~15u; }

// scrambler pattern rows of the one-launch FIXED decoders: body symbol i >= 2 sees cyc[(i - 2) mod 6]; a block whose first symbol has phase
// c0 = (i0 + 4) mod 6 sees cyc[(c0 + p) mod 6] at position p
template <class A> void scrambler_rows(A& a, const ScrCycle& sc) {
    uint8_t rows[12][16]; memset(rows, 0, sizeof rows);
    for (int r = 0; r < 11; ++r) for (int q = 0; q < 13; ++q) rows[r][q] = (uint8_t)(27u * sc.cyc[(r + q) % 6]);     // rows 0..10: the phase arrives un-reduced
    for (int q = 0; q < 13; ++q) rows[11][q] = (uint8_t)(27u * (q == 0 ? sc.pre[0] : q == 1 ? sc.pre[1] : sc.cyc[(4 + q) % 6]));   // the stream's first block: c0 = 4
    static_assert(sizeof a.pat == sizeof rows && sizeof rows == kPatBytes, "pattern rows");
    memcpy(a.pat, rows, sizeof rows);
}
}  // namespace

FusedGeom fused_geom(int k, FusedForm form) {
    const bool px = fused_px(form);
    FusedGeom g; memset(&g, 0, sizeof g);
    g.nb = fused_nb(form); g.TS = 9u * g.nb * (uint32_t)k;
    g.units_tile = px ? (g.TS / 13u) * 3u : form == FusedForm::Words ? (g.TS / 26u) * 3u : 9u * g.nb;
    const uint32_t ybytes = round16(g.TS + 16u);
    g.fma_off = px ? (uint32_t)kFx2TPx + synd_T_bytes(T3_DEC_PX_TCOP) : (uint32_t)kFx2TSeq + synd_T_bytes(32);
    g.af_off = g.fma_off + kFmaBytes; g.pat_off = g.af_off + kAfragBytes; g.y_off = g.pat_off + kPatBytes;
    if (px) {      // two symbol buffers and queues; <= kLdsThreeWgs: three workgroups per CU
        g.y_stride = ybytes; g.q_off = g.y_off + 2u * ybytes; g.q_stride = kQEntryBytes * (uint32_t)kFx2QCap;
        g.o_off = g.q_off + 2u * g.q_stride; g.lds_bytes = g.o_off + (form == FusedForm::Rgb ? 336u : 16u);
    } else {
        g.q_off = g.y_off + ybytes; g.o_off = g.q_off + kQEntryBytes * 512u;
        g.lds_bytes = g.o_off + (form == FusedForm::Words ? (g.TS / 26u) * 27u + 64u : 16u);
    }
    return g;
}

int plan_fixed_fused(uint64_t body_bytes, uint32_t hdr_syms, const t3_layout& L, const ScrCycle& sc, uint64_t units, FusedForm form, FusedPlan& p,
                     uint32_t bcn_slot, uint32_t bcn_period, uint32_t tile_lo, uint32_t tile_hi) {
    if ((L.interleave2d && form != FusedForm::Repair) || L.n_raw_words == 0 || !single_k(L)) return 1;
    const int k = L.band_k[0]; const bool px = fused_px(form), rgb = form == FusedForm::Rgb, bcn = bcn_period != 0;
    const FusedGeom g = fused_geom(k, form);
    DecFx2Args& a = p.a; memset(&a, 0, sizeof a);
    a.in_bytes = body_bytes; a.n_units = units; p.out_off = 0;
    a.k = (uint32_t)k; a.nb = g.nb; a.div_nb = to_dev(fastdiv(a.nb)); a.TS = g.TS; a.n_sym = (uint32_t)L.n_sym; a.hdr_syms = hdr_syms;
    a.n_tiles = fused_tiles(L, form);
    fill_bands(a, L, (uint64_t)tile_lo * a.nb);
    if (tile_lo || tile_hi < a.n_tiles) {
        if (!px || bcn || tile_lo >= std::min(tile_hi, a.n_tiles)) return T3_E_ARG;
        const uint64_t u0 = (uint64_t)tile_lo * g.units_tile;
        a.n_tiles = std::min(tile_hi, a.n_tiles) - tile_lo;
        p.out_off = u0 * (rgb ? 3u : 6u); a.n_units = units > u0 ? units - u0 : 0;
    }
    a.cyc24 = sc.cyc24; a.pre0 = sc.pre[0]; a.pre1 = sc.pre[1];
    scrambler_rows(a, sc);
    if (bcn) { a.bcn_slot = bcn_slot; a.bcn_pb = 9u * bcn_period - 1u; a.bcn_div = to_dev(fastdiv(a.bcn_pb)); }
    a.fma_off = g.fma_off; a.af_off = g.af_off; a.pat_off = g.pat_off; a.y_off = g.y_off; a.y_stride = g.y_stride; a.q_off = g.q_off; a.q_stride = g.q_stride;
    a.o_off = g.o_off; a.dq_off = px ? g.o_off : 0u; a.lds_bytes = g.lds_bytes;
    p.kern = {26 - k, px, rgb, bcn}; p.threads = px ? T3_DEC_PX_THREADS : 512; p.tickets = px; p.whole_frame = tile_lo == 0 && tile_hi == 0xFFFFFFFFu;
    return T3_OK;
}

int plan_fixed_uep(uint64_t body_bytes, uint32_t hdr_syms, const t3_cfg& cfg, const t3_layout& L, const ScrCycle& sc, uint64_t units, bool two_kernel, UepPlan& p) {
    if (L.n_raw_words == 0 || L.n_sym + (1u << 20) >= (1ull << 32) || body_bytes + hdr_syms >= (1ull << 32) || two_kernel) return 1;
    if (body_bytes >= (1ull << 28)) return 1;                              // the kernel packs a block's byte offset into 28 bits
    const bool il = L.interleave2d != 0 && cfg.tile_w > 1;                 // (rows of one symbol: the map is the identity)
    DecUepArgs& a = p.a; memset(&a, 0, sizeof a);
    int gk[kUepMaxGrp]; uint32_t gn[kUepMaxGrp];
    const int ng = group_bands(a, L, gk, gn);
    if (!ng) return 1;
    if (ng == 2 && gk[0] > gk[1]) {                                        // group 0 = the code with more parity (the kernel is instantiated for r0 >= r1)
        std::swap(gk[0], gk[1]); std::swap(gn[0], gn[1]);
        uint8_t t[12]; memcpy(t, a.grp[0].bands, 12); memcpy(a.grp[0].bands, a.grp[1].bands, 12); memcpy(a.grp[1].bands, t, 12);
    }
    if (il) {
        const uint64_t A = (uint64_t)cfg.tile_w * cfg.tile_h;
        if (cfg.tile_w % 4u || (A % 4u && A < L.n_sym) || std::min<uint64_t>(A, L.n_sym) < 2) return 1;   // the in-place row reversal works on dword granules (the stream's last row: bytes)
        a.il_on = 1; fill_interleave(a, cfg, L.n_sym);
    }
    uint32_t lcm = 1;
    for (int g = 0; g < ng; ++g) lcm = (uint32_t)lcm64(lcm, (uint32_t)gk[g]);
    // LDS: [hdr][fold 512][T16 1024][FMA][A operands][pattern rows 192][records 128][Y0][Y1][Q0][Q1] within kLdsThreeWgs (three workgroups per CU)
    a.fma_off = (uint32_t)kFx2TPx + synd_T_bytes(16);
    const uint32_t fixed_bytes = a.fma_off + kFmaBytes + kAfragBytes + kPatBytes + kUepRecBytes;   // (one A operand: group 0's evaluation matrix holds group 1's)
    const uint32_t budget = kLdsThreeWgs;
    uint32_t best_m = 0;
    for (uint32_t m = 1; 9u * lcm * m <= 12000u; ++m) {
        const uint32_t Lq = lcm * m, TS = 9u * Lq;
        if (TS % 4u) continue;
        uint32_t pairs = 0; bool small = false;
        for (int g = 0; g < ng; ++g) { const uint32_t nbg = Lq / (uint32_t)gk[g], items = gn[g] * nbg; if (nbg < 2u) small = true; if (nbg >= 2048u) pairs = 99; pairs += ((items + 31u) / 32u + 1u) / 2u; }
        if (small) continue;                                                              // (the kernel's divisions need two blocks per band and tile at least)
        if (pairs > 8u) break;
        // (larger tiles beat larger queues: measured on BASELINE configs[2], 0.189 ms with 9 x 1100 symbols per tile and room for 0.47 of
        // its blocks in the queues against 0.211 with 9 x 880 and room for 0.6; a block that finds its queue full is corrected on the spot)
        if (fixed_bytes + 2u * round16(TS + 16u) + 2u * kQEntryBytes * 96u + 64u > budget) break;   // (at least 96 queue entries per buffer)
        best_m = m;
    }
    if (!best_m) return 1;
    const uint32_t Lq = lcm * best_m;
    a.TS = 9u * Lq; a.n_sym = (uint32_t)L.n_sym; a.hdr_syms = hdr_syms; a.n_grp = (uint32_t)ng;
    a.in_bytes = body_bytes; a.n_units = units;
    uint32_t off = a.fma_off + kFmaBytes;
    uint64_t tiles = 0; uint32_t items_all = 0;
    for (int g = 0; g < ng; ++g) {
        auto& G = a.grp[g];
        G.r = 26u - (uint32_t)gk[g]; G.nb = Lq / (uint32_t)gk[g]; G.n_items = gn[g] * G.nb; G.div_nb = to_dev(fastdiv(G.nb));
        if (g == 0) { G.af_off = off; off += kAfragBytes; } else G.af_off = a.grp[0].af_off;
        items_all += G.n_items;
        for (uint32_t i = 0; i < gn[g]; ++i) tiles = std::max<uint64_t>(tiles, (L.band_blocks[G.bands[i]] + G.nb - 1) / G.nb);
    }
    a.n_tiles = (uint32_t)tiles;
    a.pat_off = off; off += kPatBytes; a.rec_off = off; off += kUepRecBytes;
    const uint32_t ybytes = round16(a.TS + 16u);
    a.y_off = off; a.y_stride = ybytes; off += 2u * ybytes;
    const uint32_t q_entries = std::min<uint32_t>((budget - 64u - off) / (2u * kQEntryBytes), items_all);  // per buffer, split over the groups by their share of the blocks (64: roundings below)
    uint32_t qrel = 0;
    for (int g = 0; g < ng; ++g) { auto& G = a.grp[g]; G.q_cap = std::max<uint32_t>(8u, (uint32_t)((uint64_t)q_entries * G.n_items / items_all) & ~3u); G.q_rel = qrel; qrel += kQEntryBytes * G.q_cap; }
    a.q_off = off; a.q_stride = round16(qrel); off += 2u * a.q_stride;
    a.lds_bytes = off + 16u;
    if (a.lds_bytes > 160u * 1024u) return 1;
    {   // (wave, pass) pairs of sets: pair p -> wave p % 4, pass p / 4
        for (int i = 0; i < 8; ++i) a.pair_tab[i] = 0xFFFFFFFFu;
        uint32_t pr = 0;
        for (int g = 0; g < ng; ++g) for (uint32_t it0 = 0; it0 < a.grp[g].n_items; it0 += 64u, ++pr) a.pair_tab[2u * (pr % 4u) + pr / 4u] = (uint32_t)g | it0 << 8;
    }
    fill_bands(a, L);
    scrambler_rows(a, sc);
    p.ra = 26 - gk[0]; p.rb = ng == 2 ? 26 - gk[1] : p.ra;
    return T3_OK;
}

int plan_fixed_stream(uint64_t body_bytes, uint32_t hdr_syms, const t3_cfg& cfg, const t3_layout& L, const ScrCycle& sc, uint64_t units, int to_pixels,
                      const uint32_t lut_bytes[4], StreamPlan& p) {
    if (L.n_raw_words == 0 || L.n_sym + (1u << 20) >= (1ull << 32) || body_bytes + hdr_syms >= (1ull << 32)) return 1;
    DecStArgs& a = p.a; memset(&a, 0, sizeof a);
    int gk[kStMaxGrp]; uint32_t gn[kStMaxGrp];
    const int ng = group_bands(a, L, gk, gn);                               // (four codes at most: never 0)
    uint32_t lcm = 1;
    for (int g = 0; g < ng; ++g) lcm = (uint32_t)lcm64(lcm, (uint32_t)gk[g]);
    // tile = 9 Lq stream symbols, Lq = lcm m: the m that fills the eight waves best with the tile's symbols within 16 KiB of LDS
    uint32_t best_m = 0; double best = -1.0;
    for (uint32_t m = 1; 9u * lcm * m <= 16384u; ++m) {
        uint32_t slots = 0, items = 0;
        for (int g = 0; g < ng; ++g) { const uint32_t n = gn[g] * (lcm * m / (uint32_t)gk[g]); items += n; slots += (n + 63u) / 64u; }
        const double fill = (double)items / (512.0 * ((slots + 7u) / 8u));
        if (fill > best + 1e-9) { best = fill; best_m = m; }
    }
    if (!best_m) best_m = 1;                                                // four different k: one lcm is already a large tile (LDS checked below)
    const uint32_t Lq = lcm * best_m;
    a.TS = 9u * Lq; a.n_sym = (uint32_t)L.n_sym; a.hdr_syms = hdr_syms; a.n_grp = (uint32_t)ng;
    uint32_t off = kFxLut, slots = 0; uint64_t tiles = 0;
    for (int g = 0; g < ng; ++g) {
        auto& G = a.grp[g];
        G.r = 26u - (uint32_t)gk[g]; G.nb = Lq / (uint32_t)gk[g]; G.n_items = gn[g] * G.nb; G.wave0 = slots; G.n_waves = (G.n_items + 63u) / 64u; slots += G.n_waves;
        G.lut_bytes = lut_bytes[k_index(gk[g])]; G.lut_off = off; off = round16(off + G.lut_bytes);
        for (uint32_t i = 0; i < gn[g]; ++i) tiles = std::max<uint64_t>(tiles, (L.band_blocks[G.bands[i]] + G.nb - 1) / G.nb);
    }
    a.n_slots = slots; a.n_tiles = (uint32_t)tiles;
    a.fma_off = off; a.y_off = round16(off + kFmaBytes); a.lds_bytes = a.y_off + a.TS + 64u;
    if (a.lds_bytes > 150u * 1024u) return 1;
    a.in_bytes = body_bytes;
    fill_bands(a, L);
    a.cyc24 = sc.cyc24; a.pre0 = sc.pre[0]; a.pre1 = sc.pre[1];
    EmitStArgs& e = p.e; memset(&e, 0, sizeof e);
    e.n_sym = (uint32_t)L.n_sym; e.n_units = units;
    e.span = 52u * 512u; e.n_steps = (uint32_t)((L.n_sym + e.span - 1) / e.span);
    e.il_on = L.interleave2d ? 1 : 0;
    if (e.il_on) { fill_interleave(e, cfg, L.n_sym); e.il_fast = (e.il_w % 16u == 0 && (e.il_A % 16u == 0 || e.il_A == L.n_sym)) ? 1 : 0; }
    e.sym_off = 0; e.o_off = round16(e.span + 64u);
    e.lds_bytes = e.o_off + (to_pixels ? 0u : (e.span / 26u) * 27u + 64u);
    p.to_pixels = to_pixels != 0;
    return T3_OK;
}

int plan_window(uint64_t n_raw, const t3_cfg& cfg, uint32_t fw, uint32_t fh, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, bool generic, t3_window_plan& out, t3_layout& L) {
    memset(&out, 0, sizeof out);
    if (cfg.profile == T3_RAW_MODE || fw == 0 || (uint64_t)x0 + w > fw) return T3_E_ARG;
    { const int rc = plan(n_raw, cfg, L); if (rc) return rc; }
    if ((uint64_t)w * h == 0) return T3_OK;
    const uint64_t units = 2 * n_raw;
    out.n_px = units;
    if (cfg.mode != T3_MODE_FIXED || L.interleave2d || L.beacon_on || n_raw == 0 || !single_k(L) || 9 * L.out_words >= (1ull << 32) || generic) return T3_OK;
    const uint32_t units_tile = fused_geom(L.band_k[0], FusedForm::Pixels).units_tile;      // pixel tile t produces stream pixels [t units_tile, (t + 1) units_tile)
    out.tile_range = 1; out.n_tiles = fused_tiles(L, FusedForm::Pixels);
    const uint64_t rows_end = std::min<uint64_t>((uint64_t)y0 + h, fh);                       // window rows [y0, rows_end) exist
    const uint64_t p0 = (uint64_t)y0 * fw + x0, p1 = rows_end > y0 ? std::min<uint64_t>((rows_end - 1) * fw + x0 + w, units) : 0;
    if (p0 >= p1) { out.n_px = 0; return T3_OK; }                                             // nothing of the window is in the stream: no tile
    out.tile_lo = (uint32_t)(p0 / units_tile); out.tile_hi = (uint32_t)std::min<uint64_t>((p1 + units_tile - 1) / units_tile, out.n_tiles);
    out.first_px = (uint64_t)out.tile_lo * units_tile; out.n_px = std::min<uint64_t>((uint64_t)out.tile_hi * units_tile, units) - out.first_px;
    return T3_OK;
}

int plan_frames_window(uint64_t n_raw, uint32_t n_frames, const t3_cfg& cfg, uint32_t fw, uint32_t fh, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, int out_fmt,
                       bool generic, t3_frames_window_plan& out, t3_layout& L) {
    memset(&out, 0, sizeof out);
    if ((out_fmt != 1 && out_fmt != 2) || n_frames > 65535u) return T3_E_ARG;
    { const int rc = plan_window(n_raw, cfg, fw, fh, x0, y0, w, h, generic, out.win, L); if (rc) return rc; }
    out.n_frames = n_frames;
    out.in_bytes = 9 * L.out_words; out.out_bytes = (uint64_t)w * h * (out_fmt == 2 ? 3u : 6u);
    out.in_stride_min = (out.in_bytes + 15u) & ~15ull; out.out_stride_min = (out.out_bytes + 15u) & ~15ull;
    if (out.out_bytes == 0) return T3_OK;                                                      // nothing is launched
    const t3_window_plan& wp = out.win;
    if (wp.tile_range && wp.tile_hi > wp.tile_lo && n_frames >= 2) {
        if ((uint64_t)n_frames * (wp.tile_hi - wp.tile_lo) >= (1ull << 31)) return T3_E_ARG;
        out.one_launch = 1;
        out.scratch_bytes = (uint64_t)n_frames * ((6 * wp.n_px + 15u) & ~15ull) + kWinScratchSlack;
    } else if (n_frames) out.scratch_bytes = 6 * (wp.tile_range ? wp.n_px : 2 * n_raw) + kWinScratchSlack;   // the single-frame entry's, reused frame after frame
    return T3_OK;
}

int plan_repair(uint64_t n_raw, const t3_cfg& cfg, t3_repair_plan& out, t3_layout& L) {
    memset(&out, 0, sizeof out);
    // COMPAT: the reference's parity is not a code its decoder corrects; RAW mode: no parity at all
    if (cfg.profile == T3_RAW_MODE || cfg.mode != T3_MODE_FIXED) return T3_E_ARG;
    { const int rc = plan(n_raw, cfg, L); if (rc) return rc; }
    out.in_bytes = 9 * L.out_words;
    // 2-D: the interleave acts on data symbols ahead of the band split, the blocks on the wire do not see it.  The plan keeps the decoders'
    // split all the same (plan_fixed_uep): a 2-D frame whose rows are no multiple of 4 symbols is served by the generic kernels on both sides
    const bool il_ok = !L.interleave2d || cfg.tile_w % 4u == 0;
    if (single_k(L) && !L.beacon_on && il_ok && n_raw > 0 && 9 * L.out_words < (1ull << 32)) {
        out.path = 1; out.blocks_per_tile = fused_geom(L.band_k[0], FusedForm::Repair).units_tile; out.n_tiles = fused_tiles(L, FusedForm::Repair);
    } else {
        uint64_t total = 0; for (int b = 0; b < 9; ++b) total += L.band_blocks[b];
        out.path = 0; out.blocks_per_tile = 256u; out.n_tiles = (uint32_t)((total + 255u) / 256u);
    }
    return T3_OK;
}

int plan_repair_frames(uint64_t n_raw, uint32_t n_frames, const t3_cfg& cfg, t3_repair_frames_plan& out, t3_repair_plan& P, t3_layout& L) {
    memset(&out, 0, sizeof out);
    if (n_frames > kRepairMaxFrames) return T3_E_ARG;
    { const int rc = plan_repair(n_raw, cfg, P, L); if (rc) return rc; }
    out.n_frames = n_frames; out.tiles_per_frame = P.n_tiles; out.path = P.path;
    out.one_launch = P.path == 1 && n_frames >= 2 ? 1 : 0;
    out.in_bytes = P.in_bytes; out.stride_min = P.in_bytes + (P.in_bytes & 1u);
    if (out.one_launch && (uint64_t)n_frames * P.n_tiles >= (1ull << 31)) return T3_E_ARG;     // the kernel's tile space is 32-bit (DevDiv)
    return T3_OK;
}

// the beacon the fused kernels step over in their loads (decode_body's own test)
static bool fused_beacon_ok(const t3_cfg& cfg) { return cfg.beacon_band_slot < 9 && cfg.beacon_words_period >= 2 && cfg.beacon_words_period < (1u << 27); }

int plan_decode_erasures(uint64_t n_raw, const t3_cfg& cfg, int fmt, t3_decode_erasures_plan& out, t3_layout& L) {
    memset(&out, 0, sizeof out);
    if (fmt < 0 || fmt > 2) return T3_E_ARG;
    t3_repair_plan rp;                                                     // (COMPAT, RAW mode and the framings nobody encodes: the repair's refusals)
    { const int rc = plan_repair(n_raw, cfg, rp, L); if (rc) return rc; }
    out.in_bytes = rp.in_bytes; out.out_units = fmt == 0 ? n_raw : 2 * n_raw;
    const bool fused = fmt != 0 && !L.interleave2d && single_k(L) && n_raw > 0 && 9 * L.out_words < (1ull << 32) && (!L.beacon_on || fused_beacon_ok(cfg));
    if (fused) { out.path = 1; out.n_tiles = fused_tiles(L, FusedForm::Pixels); }
    else out.scratch_bytes = (out.in_bytes + 15u) & ~15ull;
    return T3_OK;
}

int plan_fixed_era(uint64_t n_in, const t3_cfg& cfg, const t3_layout& L, const ScrCycle& sc, uint64_t units, int fmt, FusedPlan& p, uint32_t tile_lo, uint32_t tile_hi) {
    if ((fmt != 1 && fmt != 2) || (L.beacon_on && !fused_beacon_ok(cfg)) || 9 * n_in >= (1ull << 32)) return 1;
    const int rc = L.beacon_on ? plan_fixed_fused(9 * n_in, L.header_syms, L, sc, units, (FusedForm)fmt, p, cfg.beacon_band_slot, cfg.beacon_words_period, tile_lo, tile_hi)
                               : plan_fixed_fused(9 * n_in, L.header_syms, L, sc, units, (FusedForm)fmt, p, 0, 0, tile_lo, tile_hi);
    if (rc) return rc;
    DecFx2Args& a = p.a;                                                    // the queues behind the symbol buffers, widened; the output stage's tables behind them
    a.q_stride = kQEntryBytes * kEraQCap; a.o_off = a.q_off + 2u * a.q_stride; a.dq_off = a.o_off; a.lds_bytes = a.o_off + (fmt == 2 ? 336u : 16u);
    return T3_OK;
}

int plan_decode_erasures_window(uint64_t n_raw, const t3_cfg& cfg, uint32_t fw, uint32_t fh, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, int out_fmt, bool generic,
                                t3_decode_erasures_window_plan& out, t3_layout& L) {
    memset(&out, 0, sizeof out);
    if (out_fmt != 1 && out_fmt != 2) return T3_E_ARG;
    t3_decode_erasures_plan P;                                             // (COMPAT, RAW mode: its refusals)
    { const int rc = plan_decode_erasures(n_raw, cfg, out_fmt, P, L); if (rc) return rc; }
    { const int rc = plan_window(n_raw, cfg, fw, fh, x0, y0, w, h, generic, out.win, L); if (rc) { memset(&out, 0, sizeof out); return rc; } }
    out.path = P.path; out.in_bytes = P.in_bytes; out.out_bytes = (uint64_t)w * h * (out_fmt == 2 ? 3u : 6u);
    if (out.out_bytes == 0) return T3_OK;                                  // nothing is launched
    const uint64_t rows_end = std::min<uint64_t>((uint64_t)y0 + h, fh);    // window rows [y0, rows_end) exist
    out.zero_fill = (uint64_t)y0 + h > fh || (rows_end - 1) * fw + x0 + w > 2 * n_raw ? 1 : 0;    // (rows_end == 0: fh == 0, the first test)
    if (P.path == 1) out.tiles_launched = out.win.tile_range ? out.win.tile_hi - out.win.tile_lo : P.n_tiles;
    else out.scratch_bytes = P.scratch_bytes + 12 * n_raw + kWinScratchSlack;       // the copy + the frame's pixels the window is cut from
    return T3_OK;
}

int plan_decode_erasures_frames(uint64_t n_raw, uint32_t n_frames, const t3_cfg& cfg, int fmt, t3_decode_erasures_frames_plan& out, t3_layout& L) {
    memset(&out, 0, sizeof out);
    if (n_frames > kRepairMaxFrames) return T3_E_ARG;
    { const int rc = plan_decode_erasures(n_raw, cfg, fmt, out.frame, L); if (rc) { memset(&out, 0, sizeof out); return rc; } }
    const t3_decode_erasures_plan& P = out.frame;
    out.n_frames = n_frames; out.one_launch = P.path == 1 && n_frames >= 2 ? 1 : 0;
    out.in_stride_min = P.in_bytes + (P.in_bytes & 1u);
    out.out_bytes = P.out_units * (fmt == 0 ? 9u : fmt == 1 ? 6u : 3u); out.out_stride_min = (out.out_bytes + 15u) & ~15ull;
    out.scratch_bytes = out.one_launch ? 0 : P.scratch_bytes;                 // the loop reuses one frame's private copy in stream order
    if (out.one_launch && (uint64_t)n_frames * P.n_tiles >= (1ull << 31)) return T3_E_ARG;     // the kernel's tile space is 32-bit (DevDiv)
    return T3_OK;
}

int plan_decode_erasures_frames_window(uint64_t n_raw, uint32_t n_frames, const t3_cfg& cfg, uint32_t fw, uint32_t fh, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, int out_fmt,
                                       bool generic, t3_decode_erasures_frames_window_plan& out, t3_layout& L) {
    memset(&out, 0, sizeof out);
    if (n_frames > kRepairMaxFrames) return T3_E_ARG;
    { const int rc = plan_decode_erasures_window(n_raw, cfg, fw, fh, x0, y0, w, h, out_fmt, generic, out.frame, L); if (rc) { memset(&out, 0, sizeof out); return rc; } }
    const t3_decode_erasures_window_plan& P = out.frame;
    out.n_frames = n_frames; out.one_launch = P.path == 1 && n_frames >= 2 && P.tiles_launched > 0 ? 1 : 0;
    out.in_stride_min = P.in_bytes + (P.in_bytes & 1u);
    out.out_bytes = P.out_bytes; out.out_stride_min = (out.out_bytes + 15u) & ~15ull;
    out.scratch_bytes = out.one_launch ? 0 : P.scratch_bytes;                 // the loop reuses one frame's private copy in stream order
    if (out.one_launch) {
        if ((uint64_t)n_frames * P.tiles_launched >= (1ull << 31)) return T3_E_ARG;            // the kernel's ticket space is 32-bit (DevDiv)
        out.tiles_launched = n_frames * P.tiles_launched;
    }
    return T3_OK;
}

}  // namespace t3
