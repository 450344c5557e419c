// tests/cpp/enc_dispatch_demo.cpp — which encoder launches a frame gets, without a device and without libt3hip.so: built by
// tests/test_wild_inputs_lattice.py from this file, t3_enc_plan.cpp and t3_host.cpp with plain g++.  It restates the grouping of
// plan_encode (t3_api_encode.cpp, which needs the device for its tables): all nine bands in one launch when one k serves the frame or
// a table tile exists for all of them, else one launch per pair of k; per launch the matrix cores (one k / UEP) when a tile fits 512
// threads, else the table kernel.  Table sizes as tests/cpp/enc_plan_demo.cpp derives them.
// Arguments, 15 per case: profile, band_profile[0..8], tile_w, tile_h, mode, front end (0 pixels, 1 raw words, 2 RGB), n_raw_words.
// Output: one JSON list of launches per case.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "t3_enc_plan.hpp"

using namespace t3;

namespace {
struct Tables { uint32_t bytes = 0; uint32_t k_off[4] = {0, 0, 0, 0}; };
Tables tables_of(EncKind kind, uint32_t kmask, int mode) {
    Tables t; std::vector<uint32_t> afrag, img;
    for (int i = 0; i < 4; ++i) if (kmask >> i & 1) {
        if (kind == EncKind::Lut) { build_encode_lut(kOfIndex[i], mode, img); t.k_off[i] = t.bytes; t.bytes += (uint32_t)img.size() * 4u; continue; }
        build_mfma_encode(kOfIndex[i], mode, afrag, img);
        if (!t.bytes) t.bytes = (uint32_t)img.size() * 4u;
        if (kind == EncKind::Uep) { t.k_off[i] = t.bytes; t.bytes += (uint32_t)afrag.size() * 4u; }
    }
    return t;
}
const char* const kKindName[3] = {"MfmaK", "Uep", "Lut"};
}  // namespace

int main(int argc, char** argv) {
    if (argc < 16 || (argc - 1) % 15) { fprintf(stderr, "15 numbers per case\n"); return 2; }
    printf("[");
    for (int c0 = 1; c0 < argc; c0 += 15) {
        long v[15]; for (int i = 0; i < 15; ++i) v[i] = atol(argv[c0 + i]);
        t3_cfg cfg; memset(&cfg, 0, sizeof cfg);
        cfg.profile = (uint8_t)v[0]; for (int b = 0; b < 9; ++b) cfg.band_profile[b] = (uint8_t)v[1 + b];
        cfg.tile_w = (uint16_t)v[10]; cfg.tile_h = (uint16_t)v[11]; cfg.mode = (uint8_t)v[12];
        cfg.seed_a = cfg.seed_b = cfg.seed_s0 = 1; cfg.superframe_words = 8192; cfg.subword = 27; cfg.centered = 1;
        const int fe = (int)v[13];
        t3_layout L; if (plan((uint64_t)v[14], cfg, L) != T3_OK) { fprintf(stderr, "plan failed\n"); return 2; }
        uint32_t kmask = 0; for (int b = 0; b < 9; ++b) kmask |= 1u << k_index(L.band_k[b]);
        const bool one_k = (kmask & (kmask - 1)) == 0;
        uint32_t groups[2] = {0x1FFu, 0u}; int n = 1;
        if (!one_k) {
            const Tables t = tables_of(EncKind::Lut, kmask, cfg.mode); EncLaunch probe;
            if (!plan_enc_group(L, cfg, 0x1FF, fe, t.bytes, t.k_off, EncKind::Lut, probe)) {
                uint32_t per_k[4] = {0, 0, 0, 0}, m = 0;
                for (int i = 0; i < 4; ++i) if (kmask >> i & 1) { for (int b = 0; b < 9; ++b) if (k_index(L.band_k[b]) == i) per_k[m] |= 1u << b; ++m; }
                groups[0] = m == 2 ? per_k[0] : per_k[0] | per_k[1]; groups[1] = m == 2 ? per_k[1] : per_k[2] | per_k[3]; n = 2;
            }
        }
        printf("%s[", c0 > 1 ? ",\n" : "");
        for (int g = 0; g < n; ++g) {
            const uint32_t m = groups[g]; uint32_t km = 0;
            for (int b = 0; b < 9; ++b) if (m >> b & 1) km |= 1u << k_index(L.band_k[b]);
            const EncKind first = one_k ? EncKind::MfmaK : EncKind::Uep;
            Tables t = tables_of(first, km, cfg.mode); EncLaunch e; memset(&e, 0, sizeof e);
            bool found = plan_enc_group(L, cfg, m, fe, t.bytes, t.k_off, first, e) && e.block <= 512;
            if (!found) { t = tables_of(EncKind::Lut, km, cfg.mode); found = plan_enc_group(L, cfg, m, fe, t.bytes, t.k_off, EncKind::Lut, e); }
            if (!found) { fprintf(stderr, "no tile\n"); return 2; }
            printf("%s{\"mask\":%u,\"kind\":\"%s\",\"block\":%u,\"tile\":%u,\"n_tiles\":%u,\"il_on\":%u,\"il_async\":%u,\"il_w\":%u}", g ? "," : "", m, kKindName[(int)e.kind], e.block,
                   9u * e.a.Lq, e.a.n_tiles, e.a.il_on, e.a.il_async, e.a.il_w);
        }
        printf("]");
    }
    printf("]\n");
    return 0;
}
