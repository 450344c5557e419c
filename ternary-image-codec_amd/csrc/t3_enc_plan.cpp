// t3_enc_plan.cpp — the encoder's tile planner (t3_enc_plan.hpp).  Host arithmetic only.
#include "t3_enc_plan.hpp"

#include <string.h>

#include <algorithm>

namespace t3 {
namespace {
uint32_t round16(uint32_t x) { return (x + 15u) & ~15u; }

// Phase 1 gives a lane four consecutive input triples of `unit` symbols each: waves that cover the worst-placed tile of TS symbols (tile
// starts cycle through S0 mod `cycle`).  Pixels: 52, 13; raw words (1-D, convert_words_packed: 104 symbols per lane): 104, 26
uint32_t p1_waves(uint32_t TS, uint32_t cycle, uint32_t unit) {
    uint32_t worst = 0;
    for (uint32_t t = 0; t < cycle; ++t) {
        const uint64_t S0 = (uint64_t)t * TS;
        const uint64_t t_base = (S0 / unit) & ~3ull, t_end = (S0 + TS + unit - 1) / unit;
        worst = std::max<uint32_t>(worst, (uint32_t)((t_end - t_base + 3) / 4));
    }
    return (worst + 63) / 64;
}

// The tile of Lq data symbols per band: its work and its LDS carve-up [hdr][tables][symbols][stage 0][stage 1][RGB: chroma quantiser]
struct TileGeom {
    uint32_t Lq, sym_off, stage_off, stage_stride, stage_groups, n_stage, qt_off, lds_bytes;
    uint32_t waves, p1_wpp;                                // phase 2: waves of blocks; phase 1: waves that cover the tile (set when it fits)
    uint32_t grp_items[4], n_sets;                         // blocks of the bands of each k index, and their sets of 32 (UEP)
    bool fits;                                             // within the pass's LDS budget and wave limit (UEP: and the set table)
};

}  // namespace

// UEP on the matrix cores: bands are grouped by k, a group's blocks of a tile are dealt linearly into sets of 32; eight waves take two sets each
bool plan_enc_group(const t3_layout& L, const t3_cfg& cfg, uint32_t band_mask, int fe, uint32_t lut_bytes, const uint32_t k_off[4], EncKind kind, EncLaunch& out) {
    EncArgs& a = out.a; memset(&a, 0, sizeof a);
    const bool grp = kind == EncKind::Uep;
    const bool il2d = L.interleave2d && cfg.tile_w > 1;                  // rows of one symbol: the boustrophedon map is the identity (and the kernels' row divisions assume >= 2)
    const uint32_t GS = fe_px(fe) ? kGroupSyms : kGroupSymsW, GB = fe == FE_PIXELS ? kGroupBytes : fe == FE_RGB ? kGroupBytesRgb : kGroupBytesW;
    uint64_t Lk = 2;
    for (int b = 0; b < 9; ++b) if (band_mask >> b & 1) Lk = lcm64(Lk, L.band_k[b]);
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
    // the one place that sizes a tile: the search below scores what it returns, the arguments are filled from the tile picked
    const auto tile_geom = [&](uint32_t Lq, uint32_t budget, uint32_t max_waves) {
        TileGeom g{};
        const uint32_t TS = 9u * Lq;
        g.Lq = Lq;
        uint32_t blocks = 0;
        for (int b = 0; b < 9; ++b) if (band_mask >> b & 1) { const uint32_t nb = Lq / L.band_k[b]; blocks += nb; g.grp_items[k_index(L.band_k[b])] += nb; }
        for (uint32_t items : g.grp_items) g.n_sets += (items + 31) / 32;
        g.waves = grp ? 8u : (blocks + 63) / 64;               // lanes are dealt to blocks linearly across bands; UEP: always 512 threads
        g.sym_off = hdr + round16(lut_bytes) + sym_front;
        g.stage_off = g.sym_off + round16(TS + il_extra) + sym_back;   // slack either side: phase 1 writes whole pixel triples / whole lanes of word triples
        g.stage_groups = (TS + il_extra) / GS + 8;
        uint32_t stage = g.stage_groups * GB + 1024 + 32 + il_stage;   // +1 KiB: LDS-DMA pieces are whole
        if (il_async == 1u) stage = std::max(stage, TS + 64u);         // the permutation pass writes the tile's 9 Lq symbols into the consumed stage buffer (RGB input is smaller than that)
        g.stage_stride = round16(stage);
        g.n_stage = il2d && !il_async ? 1u : 2u;                       // pipelined flow: two stage buffers (the next tile streams in early)
        g.lds_bytes = g.stage_off + g.n_stage * g.stage_stride;
        if (fe == FE_RGB) { g.qt_off = g.lds_bytes; g.lds_bytes += 256u; }   // chroma quantiser table of the fused bridge
        g.fits = g.lds_bytes <= budget && g.waves <= max_waves && (!grp || g.n_sets <= (uint32_t)kMaxSets);
        if (g.fits) g.p1_wpp = words_packed ? p1_waves(TS, 104, 26) : p1_waves(TS + il_extra + (il_async == 2u ? 312u : 0u), 52, 13);   // (three runs: up to six lane units of rounding)
        return g;
    };
    // pick q: tile = 9*Lk*q stream symbols; band b then owns Lk*q/k_b blocks
    double best_score = -1; TileGeom g{};                                 // g.Lq == 0: none yet
    for (int pass = 0; pass < 2 && !g.Lq; ++pass) {
        if (grp && pass > 0) break;                                      // the UEP kernel: always 512 threads, three workgroups per CU
        const uint32_t budget = pass == 0 ? kLdsThreeWgs : 160u * 1024u, max_waves = pass == 0 ? 8u : (uint32_t)kMaxWaves;   // pass 0: 512-thread workgroups, three per CU
        for (uint32_t q = 1; q <= 4096; ++q) {
            if (mixed && !grp && (q & 1u)) continue;                     // mixed k, LUT kernel: even multipliers only (measured: odd ones halve its speed)
            const uint64_t Lq = Lk * q; if (9 * Lq > 60000) break;
            const TileGeom c = tile_geom((uint32_t)Lq, budget, max_waves); if (!c.fits) break;
            const uint32_t waves = c.waves, wpp = c.p1_wpp;
            if ((fe_px(fe) || words_packed) && (words_packed ? 2u : 1u) * wpp > std::max(waves, 4u)) continue;   // phase 1 has the workgroup's waves, no more
            // wave-instructions per stream symbol: phase 2 costs ~180 per wave, phase 1 (pixels) ~120 per wave-iteration
            // UEP kernel: the phases are barrier-separated and a wave runs its sets one after the other, so a tile costs one
            // phase-1 pass plus ceil(sets / 8) set times, whatever the number of busy waves
            // + a fixed cost per tile (barriers, ticket, prefetch issue, the runs' rounding in 2-D): without it the model preferred tiles of
            // 5 full waves to larger ones of 7-8 partly filled waves, measured 2-12 % slower (profiles/r03/notes.md: tile sweeps)
            const double cost = grp ? (220.0 + 100.0 * ((c.n_sets + 7) / 8)) / (double)(9 * Lq)
                                    : (600.0 + 180.0 * waves + (fe_px(fe) ? 220.0 * wpp : words_packed ? 250.0 * wpp : 180.0 * waves)) / (double)(9 * Lq);
            const double score = 1.0 / cost + 1e-9 * (double)Lq;
            if (score > best_score) { best_score = score; g = c; }
        }
    }
    if (!g.Lq) return false;
    const uint32_t Lq = g.Lq;
    a.Lq = Lq; a.lut_bytes = round16(lut_bytes);
    a.sym_off = g.sym_off; a.stage_off = g.stage_off; a.stage_groups = g.stage_groups; a.stage_stride = g.stage_stride;
    a.lds_bytes = g.lds_bytes; a.qt_off = g.qt_off; a.p1_wpp = g.p1_wpp; a.il_async = il_async;
    uint32_t n_tiles = 0;
    fill_bands(a, L);
    for (int b = 0; b < 9; ++b) {
        a.band_k[b] = L.band_k[b];
        a.band_lut_off[b] = hdr + k_off[k_index(L.band_k[b])];
        if (!(band_mask >> b & 1)) { a.band_nb_tile[b] = 0; a.band_blocks[b] = 0; continue; }
        const uint32_t nb = Lq / L.band_k[b];
        a.band_nb_tile[b] = nb;
        n_tiles = std::max<uint32_t>(n_tiles, (uint32_t)((L.band_blocks[b] + nb - 1) / nb));
    }
    a.n_tiles = n_tiles;
    { uint32_t acc = 0; for (int b = 0; b < 9; ++b) { a.band_first[b] = acc; acc += a.band_nb_tile[b]; } a.band_first[9] = a.n_items = acc; }
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
    out.kind = kind; out.block = 64u * std::max(g.waves, 4u);
    a.nb_uniform = !mixed && band_mask == 0x1FF ? a.band_nb_tile[0] : 0u; a.div_nb = to_dev(fastdiv(a.nb_uniform ? a.nb_uniform : 1u));
    if (grp) {
        uint32_t ng = 0, ns = 0;
        for (int i = 0; i < 4; ++i) {
            if (!g.grp_items[i]) continue;
            EncArgs::Grp& G = a.grp[ng];
            uint32_t nbands = 0;
            for (int b = 0; b < 9; ++b) if ((band_mask >> b & 1) && k_index(L.band_k[b]) == i) G.bands[nbands++] = (uint8_t)b;
            G.nb = Lq / (uint32_t)kOfIndex[i]; G.div_nb = to_dev(fastdiv(G.nb)); G.n_items = g.grp_items[i]; G.r = 26u - (uint32_t)kOfIndex[i];
            G.afrag_off = hdr + k_off[i];
            mfma_scrambler_table(kOfIndex[i], sc, G.scr);
            for (uint32_t it0 = 0; it0 < G.n_items; it0 += 32) a.set_tab[ns++] = ng | it0 << 8;
            ++ng;
        }
        a.n_grp = ng; a.n_sets = g.n_sets;
    }
    return true;
}

}  // namespace t3
