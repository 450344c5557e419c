// tests/cpp/enc_plan_demo.cpp — the encoder's tile planner (csrc/t3_enc_plan.cpp) on a fixed list of cases, without a device and without
// libt3hip.so: built by tests/test_enc_plan.py from this file, t3_enc_plan.cpp and t3_host.cpp with plain g++.  One JSON record per case on
// stdout: whether a tile was found, the kernel kind, the workgroup size and every field of EncArgs the planner sets (the pointers, hdr,
// the beacon fields and dbg are the launch side's).  The test compares them with tests/golden/enc_plan.json, recorded from the planner
// as it was before it had a unit of its own.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "t3_enc_plan.hpp"

using namespace t3;

namespace {

// The byte size and per-k offsets of the tables a launch of `kind` stages for the k's of kmask, as the library's table caches lay them out
struct Tables { uint32_t bytes = 0; uint32_t k_off[4] = {0, 0, 0, 0}; };
Tables tables_of(EncKind kind, uint32_t kmask, int mode) {
    Tables t; std::vector<uint32_t> afrag, img;
    for (int i = 0; i < 4; ++i) if (kmask >> i & 1) {
        if (kind == EncKind::Lut) { build_encode_lut(kOfIndex[i], mode, img); t.k_off[i] = t.bytes; t.bytes += (uint32_t)img.size() * 4u; continue; }
        build_mfma_encode(kOfIndex[i], mode, afrag, img);
        if (!t.bytes) t.bytes = (uint32_t)img.size() * 4u;                   // the T and M tables: once
        if (kind == EncKind::Uep) { t.k_off[i] = t.bytes; t.bytes += (uint32_t)afrag.size() * 4u; }
    }
    return t;
}

template <class T> void arr(const char* name, const T* v, int n) {
    printf(",\"%s\":[", name);
    for (int i = 0; i < n; ++i) printf("%s%llu", i ? "," : "", (unsigned long long)v[i]);
    printf("]");
}
void num(const char* name, uint64_t v) { printf(",\"%s\":%llu", name, (unsigned long long)v); }
void div3(const char* name, const DevDiv& d) { const uint32_t v[3] = {d.mul, d.sh, d.d}; arr(name, v, 3); }

struct Frame { const char* name; uint8_t k[9]; };
const Frame kOneK[4] = {{"k24", {24, 24, 24, 24, 24, 24, 24, 24, 24}}, {"k22", {22, 22, 22, 22, 22, 22, 22, 22, 22}},
                        {"k20", {20, 20, 20, 20, 20, 20, 20, 20, 20}}, {"k18", {18, 18, 18, 18, 18, 18, 18, 18, 18}}};
const Frame kTwoK = {"k22k24", {22, 22, 22, 24, 24, 24, 24, 24, 24}}, kThreeK = {"k18k22k24", {18, 18, 18, 22, 22, 22, 24, 24, 24}},
            kFourK = {"k18k20k22k24", {18, 18, 20, 20, 22, 22, 24, 24, 24}};
const char* const kFeName[3] = {"px", "words", "rgb"};      // FE_PIXELS, FE_WORDS, FE_RGB
const char* const kKindName[3] = {"MfmaK", "Uep", "Lut"};

t3_cfg cfg_of(const Frame& f, uint32_t tile_w, int mode = T3_MODE_FIXED) {
    t3_cfg c; memset(&c, 0, sizeof c);
    c.profile = tile_w ? T3_P5_RS26_22_2D : T3_P2_RS26_22; c.mode = (uint8_t)mode;
    for (int b = 0; b < 9; ++b) c.band_profile[b] = (uint8_t)k_index(f.k[b]);
    c.tile_w = (uint16_t)tile_w; c.tile_h = tile_w ? 64 : 0;
    c.seed_a = c.seed_b = c.seed_s0 = 1; c.superframe_words = 8192; c.subword = 27; c.centered = 1;
    return c;
}

int n_cases = 0;
// One record: a launch over the bands whose k index is in `kidx` (0xF: all nine), planned from the tables of those k.
void run(const Frame& f, int fe, EncKind kind, uint64_t n_raw, uint32_t tile_w = 0, uint32_t kidx = 0xF, const t3_cfg* given = nullptr) {
    const t3_cfg cfg = given ? *given : cfg_of(f, tile_w);
    t3_layout L; if (plan(n_raw, cfg, L) != T3_OK) { fprintf(stderr, "plan failed\n"); exit(2); }
    uint32_t mask = 0, kmask = 0;
    for (int b = 0; b < 9; ++b) if (kidx >> k_index(L.band_k[b]) & 1) { mask |= 1u << b; kmask |= 1u << k_index(L.band_k[b]); }
    const Tables t = tables_of(kind, kmask, cfg.mode);
    EncLaunch e; memset(&e, 0, sizeof e);
    const bool found = plan_enc_group(L, cfg, mask, fe, t.bytes, t.k_off, kind, e);
    printf("%s{\"case\":\"%s %s %s mask=%03x w=%u n=%llu%s\",\"found\":%d,\"want_kind\":\"%s\"", n_cases++ ? ",\n" : "", f.name, kFeName[fe], kKindName[(int)kind], mask, tile_w,
           (unsigned long long)n_raw, given ? " cfg" : "", found ? 1 : 0, kKindName[(int)kind]);
    if (found) {
        const EncArgs& a = e.a;
        printf(",\"kind\":\"%s\"", kKindName[(int)e.kind]); num("block", e.block);
        num("lut_bytes", a.lut_bytes); num("n_sym", a.n_sym); num("n_tiles", a.n_tiles); num("Lq", a.Lq);
        arr("band_k", a.band_k, 9); arr("band_nb_tile", a.band_nb_tile, 9); arr("band_blocks", a.band_blocks, 9); arr("band_lut_off", a.band_lut_off, 9);
        arr("band_boff6", a.band_boff6, 9); arr("band_body_off", a.band_body_off, 9); arr("band_first", a.band_first, 10);
        num("n_items", a.n_items); num("nb_uniform", a.nb_uniform); div3("div_nb", a.div_nb);
        num("sym_off", a.sym_off); num("stage_off", a.stage_off); num("lds_bytes", a.lds_bytes); num("stage_stride", a.stage_stride); num("stage_groups", a.stage_groups);
        num("cyc24", a.cyc24); num("pre0", a.pre0); num("pre1", a.pre1); arr("scr", a.scr, 12);
        printf(",\"grp\":[");
        for (int g = 0; g < kMaxGrp; ++g) {
            const EncArgs::Grp& G = a.grp[g];
            printf("%s{\"nb\":%u", g ? "," : "", G.nb); div3("div_nb", G.div_nb); num("n_items", G.n_items); num("r", G.r); arr("bands", G.bands, 12);
            num("afrag_off", G.afrag_off); arr("scr", G.scr, 12); printf("}");
        }
        printf("]"); num("n_grp", a.n_grp); num("n_sets", a.n_sets); arr("set_tab", a.set_tab, kMaxSets);
        num("il_on", a.il_on); num("il_w", a.il_w); num("il_A", a.il_A); num("il_async", a.il_async); div3("div_A", a.div_A); div3("div_w", a.div_w);
        num("p1_wpp", a.p1_wpp); num("qt_off", a.qt_off);
    }
    printf("}");
}

}  // namespace

int main() {
    const int fes[3] = {FE_PIXELS, FE_WORDS, FE_RGB};
    const uint64_t kMid = 100003, k8K = 7680ull * 4320ull / 2;
    printf("[");
    // one k on all nine bands: the single-k matrix-core kernel, every code and front end
    for (const Frame& f : kOneK) for (int fe : fes) run(f, fe, EncKind::MfmaK, kMid);
    // 2-D: a row of one symbol (the identity: il_on 0), the staged and the two pipelined flows either side of 512, a wide row
    for (uint32_t w : {1u, 2u, 512u, 513u, 4096u}) for (int fe : fes) run(kOneK[1], fe, EncKind::MfmaK, kMid, w);
    for (uint32_t w : {2u, 513u}) for (int fe : fes) for (EncKind kind : {EncKind::Uep, EncKind::Lut}) run(kTwoK, fe, kind, kMid, w);
    // several k: all nine bands, each k's bands, each pair of k's -- on the matrix cores and as LUT launches.  Four k, all bands, LUT: no tile
    // (lcm 3960, even multipliers only: 9 Lq > 60000), which is why a frame's launches are split by k
    for (const Frame* f : {&kTwoK, &kThreeK, &kFourK}) {
        uint32_t ks = 0; for (int b = 0; b < 9; ++b) ks |= 1u << k_index(f->k[b]);
        for (EncKind kind : {EncKind::Uep, EncKind::Lut}) {
            for (int fe : fes) run(*f, fe, kind, kMid);
            for (int i = 0; i < 4; ++i) if (ks >> i & 1) run(*f, FE_PIXELS, kind, kMid, 0, 1u << i);
            for (int i = 0; i < 4; ++i) for (int j = i + 1; j < 4; ++j)
                if ((ks >> i & 1) && (ks >> j & 1) && (1u << i | 1u << j) != ks) run(*f, FE_PIXELS, kind, kMid, 0, 1u << i | 1u << j);
        }
    }
    // frame sizes: nothing, one word, one tile of blocks in every band (k = 22, pixels: 49 blocks), one block more, an 8K frame
    for (uint64_t n : {0ull, 1ull, 1119ull, 1120ull, (unsigned long long)k8K}) run(kOneK[1], FE_PIXELS, EncKind::MfmaK, n);
    for (uint64_t n : {0ull, 1ull, (unsigned long long)k8K}) { run(kOneK[2], FE_WORDS, EncKind::MfmaK, n); run(kThreeK, FE_RGB, EncKind::Uep, n); }
    run(kTwoK, FE_PIXELS, EncKind::Lut, k8K); run(kOneK[0], FE_RGB, EncKind::MfmaK, k8K, 513);
    // the reference's framing (a band's tail dropped) and other scrambler seeds
    { t3_cfg c = cfg_of(kOneK[3], 0, T3_MODE_COMPAT); run(kOneK[3], FE_PIXELS, EncKind::MfmaK, kMid, 0, 0xF, &c); }
    { t3_cfg c = cfg_of(kThreeK, 0); c.seed_a = 5; c.seed_b = 7; c.seed_s0 = 11; run(kThreeK, FE_PIXELS, EncKind::Uep, kMid, 0, 0xF, &c); }
    printf("]\n");
    fprintf(stderr, "%d cases\n", n_cases);
    return 0;
}
