// tests/cpp/dec_plan_demo.cpp — the decode side's planner (csrc/t3_dec_plan.cpp) on a fixed list of cases, without a device and without
// libt3hip.so: built by tests/test_dec_plan.py from this file, t3_dec_plan.cpp and t3_host.cpp with plain g++.  One JSON record per case on
// stdout: the return code and, for a plan found, the kernel value and every field of the argument blocks the planner sets (the table,
// stream and output pointers, tickets, verdict and header fields, edge / ystream and dbg are the launch side's); for the host-arithmetic
// plans every field of the plan.  The test compares them with tests/golden/dec_plan.json, recorded from the planners as they were
// before they had a unit of their own.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "t3_dec_plan.hpp"

using namespace t3;

namespace {

template <class T> void arr(const char* name, const T* v, int n) {
    printf(",\"%s\":[", name);
    for (int i = 0; i < n; ++i) printf("%s%llu", i ? "," : "", (unsigned long long)v[i]);
    printf("]");
}
void num(const char* name, uint64_t v) { printf(",\"%s\":%llu", name, (unsigned long long)v); }
void div3(const char* name, const DevDiv& d) { const uint32_t v[3] = {d.mul, d.sh, d.d}; arr(name, v, 3); }
template <class A> void bands(const A& a) { arr("band_blocks", a.band_blocks, 9); arr("band_body_off", a.band_body_off, 9); arr("band_boff6", a.band_boff6, 9); }

int n_cases = 0;
void open(const char* kind, const char* name, int rc) { printf("%s{\"case\":\"%s %s\",\"rc\":%d", n_cases++ ? ",\n" : "", kind, name, rc); }

t3_cfg cfg_of(const uint8_t k[9], uint32_t tile_w = 0, uint32_t tile_h = 64, int mode = T3_MODE_FIXED) {
    t3_cfg c; memset(&c, 0, sizeof c);
    c.profile = tile_w ? T3_P5_RS26_22_2D : T3_P2_RS26_22; c.mode = (uint8_t)mode;
    for (int b = 0; b < 9; ++b) c.band_profile[b] = (uint8_t)k_index(k[b]);
    c.tile_w = (uint16_t)tile_w; c.tile_h = (uint16_t)(tile_w ? tile_h : 0);
    c.seed_a = c.seed_b = c.seed_s0 = 1; c.superframe_words = 8192; c.subword = 27; c.centered = 1;
    return c;
}
t3_cfg cfg_k(int k, uint32_t tile_w = 0, uint32_t tile_h = 64, int mode = T3_MODE_FIXED) { const uint8_t ks[9] = {(uint8_t)k, (uint8_t)k, (uint8_t)k, (uint8_t)k, (uint8_t)k, (uint8_t)k, (uint8_t)k, (uint8_t)k, (uint8_t)k}; return cfg_of(ks, tile_w, tile_h, mode); }
t3_cfg with_beacon(t3_cfg c, uint32_t period, uint32_t slot) { c.beacon_words_period = period; c.beacon_band_slot = (uint8_t)slot; c.beacon_enabled = 1; return c; }
t3_layout layout(uint64_t n_raw, const t3_cfg& c) { t3_layout L; if (plan(n_raw, c, L) != T3_OK) { fprintf(stderr, "plan failed\n"); exit(2); } return L; }
ScrCycle cycle(const t3_cfg& c) { const ScrCycle s0 = scrambler_cycle(c.seed_a, c.seed_b, c.seed_s0); return scrambler_cycle_from_next(s0.next, c.seed_s0); }

const char* const kForm[4] = {"words", "px", "rgb", "repair"};

// the fused decoder as decode_body asks for it: on the framed stream with the beacon stepped over (bcn), else on the body
void fused(const char* name, const t3_cfg& c, uint64_t n_raw, FusedForm form, bool bcn = false, uint32_t lo = 0, uint32_t hi = 0xFFFFFFFFu) {
    const t3_layout L = layout(n_raw, c);
    const uint64_t units = form == FusedForm::Words ? n_raw : form == FusedForm::Repair ? 0 : 2 * n_raw;
    FusedPlan p; memset(&p, 0, sizeof p);
    const int rc = bcn ? plan_fixed_fused(9 * L.out_words, L.header_syms, L, cycle(c), units, form, p, c.beacon_band_slot, c.beacon_words_period, lo, hi)
                       : plan_fixed_fused(L.beacon_on ? L.body_syms : 9 * L.out_words, L.beacon_on ? 0u : L.header_syms, L, cycle(c), units, form, p, 0, 0, lo, hi);
    char nm[160]; snprintf(nm, sizeof nm, "%s %s w=%u n=%llu period=%u slot=%u bcn=%d lo=%u hi=%u", name, kForm[(int)form], c.tile_w, (unsigned long long)n_raw, c.beacon_words_period, c.beacon_band_slot, bcn ? 1 : 0, lo, hi);
    open("fused", nm, rc);
    if (rc == T3_OK) {
        const DecFx2Args& a = p.a;
        num("r", (uint64_t)p.kern.r); num("px", p.kern.px); num("rgb", p.kern.rgb); num("bcn", p.kern.bcn); num("threads", p.threads); num("tickets", p.tickets); num("whole_frame", p.whole_frame);
        num("out_off", p.out_off); num("in_bytes", a.in_bytes); num("n_units", a.n_units); num("fma_off", a.fma_off);
        num("k", a.k); num("nb", a.nb); num("n_tiles", a.n_tiles); num("TS", a.TS); div3("div_nb", a.div_nb); num("n_sym", a.n_sym); num("hdr_syms", a.hdr_syms); bands(a);
        num("cyc24", a.cyc24); num("pre0", a.pre0); num("pre1", a.pre1); arr("pat", a.pat, 48); num("pat_off", a.pat_off);
        num("y_off", a.y_off); num("y_stride", a.y_stride); num("q_off", a.q_off); num("q_stride", a.q_stride); num("o_off", a.o_off); num("af_off", a.af_off); num("lds_bytes", a.lds_bytes);
        num("bcn_slot", a.bcn_slot); num("bcn_pb", a.bcn_pb); div3("bcn_div", a.bcn_div); num("dq_off", a.dq_off);
        const FusedGeom g = fused_geom((int)a.k, form);
        num("g_units_tile", g.units_tile); num("g_tiles", fused_tiles(L, form));
    }
    printf("}");
}

void uep(const char* name, const t3_cfg& c, uint64_t n_raw, bool two_kernel = false, uint64_t body_bytes = 0) {
    const t3_layout L = layout(n_raw, c);
    UepPlan p; memset(&p, 0, sizeof p);
    const int rc = plan_fixed_uep(body_bytes ? body_bytes : 9 * L.out_words, L.header_syms, c, L, cycle(c), 2 * n_raw, two_kernel, p);
    char nm[160]; snprintf(nm, sizeof nm, "%s w=%u h=%u n=%llu two=%d body=%llu", name, c.tile_w, c.tile_h, (unsigned long long)n_raw, two_kernel ? 1 : 0, (unsigned long long)body_bytes);
    open("uep", nm, rc);
    if (rc == T3_OK) {
        const DecUepArgs& a = p.a;
        num("ra", (uint64_t)p.ra); num("rb", (uint64_t)p.rb); num("in_bytes", a.in_bytes); num("n_units", a.n_units); num("fma_off", a.fma_off);
        printf(",\"grp\":[");
        for (int g = 0; g < kUepMaxGrp; ++g) {
            const DecUepArgs::Grp& G = a.grp[g];
            printf("%s{\"r\":%u", g ? "," : "", G.r); num("nb", G.nb); num("n_items", G.n_items); num("af_off", G.af_off); num("q_rel", G.q_rel); num("q_cap", G.q_cap); div3("div_nb", G.div_nb);
            arr("bands", G.bands, 12); printf("}");
        }
        printf("]"); num("n_grp", a.n_grp); arr("pair_tab", a.pair_tab, 8);
        num("TS", a.TS); num("n_tiles", a.n_tiles); num("n_sym", a.n_sym); num("hdr_syms", a.hdr_syms); bands(a);
        arr("pat", a.pat, 48); num("pat_off", a.pat_off); num("rec_off", a.rec_off);
        num("y_off", a.y_off); num("y_stride", a.y_stride); num("q_off", a.q_off); num("q_stride", a.q_stride); num("lds_bytes", a.lds_bytes);
        num("il_on", a.il_on); num("il_w", a.il_w); num("il_A", a.il_A); div3("div_A", a.div_A); div3("div_w", a.div_w);
    }
    printf("}");
}

uint32_t kLutBytes[4];
void stream(const char* name, const t3_cfg& c, uint64_t n_raw, int to_pixels) {
    const t3_layout L = layout(n_raw, c);
    StreamPlan p; memset(&p, 0, sizeof p);
    const int rc = plan_fixed_stream(9 * L.out_words, L.header_syms, c, L, cycle(c), to_pixels ? 2 * n_raw : n_raw, to_pixels, kLutBytes, p);
    char nm[160]; snprintf(nm, sizeof nm, "%s w=%u h=%u n=%llu %s", name, c.tile_w, c.tile_h, (unsigned long long)n_raw, kForm[to_pixels]);
    open("stream", nm, rc);
    if (rc == T3_OK) {
        const DecStArgs& a = p.a; const EmitStArgs& e = p.e;
        num("to_pixels", p.to_pixels); num("in_bytes", a.in_bytes); num("fma_off", a.fma_off);
        printf(",\"grp\":[");
        for (int g = 0; g < kStMaxGrp; ++g) {
            const DecStArgs::Grp& G = a.grp[g];
            printf("%s{\"r\":%u", g ? "," : "", G.r); num("nb", G.nb); num("n_items", G.n_items); num("wave0", G.wave0); num("n_waves", G.n_waves); num("lut_off", G.lut_off); num("lut_bytes", G.lut_bytes);
            arr("bands", G.bands, 12); printf("}");
        }
        printf("]"); num("n_grp", a.n_grp); num("n_slots", a.n_slots); num("n_tiles", a.n_tiles); num("TS", a.TS); num("n_sym", a.n_sym); num("hdr_syms", a.hdr_syms); bands(a);
        num("cyc24", a.cyc24); num("pre0", a.pre0); num("pre1", a.pre1); num("y_off", a.y_off); num("lds_bytes", a.lds_bytes);
        num("e_n_sym", e.n_sym); num("e_n_units", e.n_units); num("e_span", e.span); num("e_n_steps", e.n_steps);
        num("e_il_on", e.il_on); num("e_il_w", e.il_w); num("e_il_A", e.il_A); num("e_il_fast", e.il_fast); div3("e_div_A", e.div_A); div3("e_div_w", e.div_w);
        num("e_sym_off", e.sym_off); num("e_o_off", e.o_off); num("e_lds_bytes", e.lds_bytes);
    }
    printf("}");
}

void win_fields(const t3_window_plan& p) { num("n_tiles", p.n_tiles); num("tile_lo", p.tile_lo); num("tile_hi", p.tile_hi); num("first_px", p.first_px); num("n_px", p.n_px); num("tile_range", p.tile_range); }
void window(const char* name, const t3_cfg& c, uint64_t n_raw, uint32_t fw, uint32_t fh, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, bool generic = false) {
    t3_window_plan p; t3_layout L;
    const int rc = plan_window(n_raw, c, fw, fh, x0, y0, w, h, generic, p, L);
    char nm[200]; snprintf(nm, sizeof nm, "%s n=%llu %ux%u at %u,%u %ux%u generic=%d", name, (unsigned long long)n_raw, fw, fh, x0, y0, w, h, generic ? 1 : 0);
    open("window", nm, rc); win_fields(p); printf("}");
}
void frames_window(const char* name, const t3_cfg& c, uint64_t n_raw, uint32_t n, uint32_t fw, uint32_t fh, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, int fmt, bool generic = false) {
    t3_frames_window_plan p; t3_layout L;
    const int rc = plan_frames_window(n_raw, n, c, fw, fh, x0, y0, w, h, fmt, generic, p, L);
    char nm[200]; snprintf(nm, sizeof nm, "%s n=%llu frames=%u %ux%u at %u,%u %ux%u fmt=%d generic=%d", name, (unsigned long long)n_raw, n, fw, fh, x0, y0, w, h, fmt, generic ? 1 : 0);
    open("frames_window", nm, rc); win_fields(p.win);
    num("n_frames", p.n_frames); num("one_launch", p.one_launch); num("in_bytes", p.in_bytes); num("out_bytes", p.out_bytes); num("in_stride_min", p.in_stride_min);
    num("out_stride_min", p.out_stride_min); num("scratch_bytes", p.scratch_bytes); printf("}");
}
void repair(const char* name, const t3_cfg& c, uint64_t n_raw, uint32_t n_frames) {
    t3_repair_frames_plan fp; t3_repair_plan P; t3_layout L; memset(&P, 0, sizeof P);
    const int rc = plan_repair_frames(n_raw, n_frames, c, fp, P, L);
    char nm[160]; snprintf(nm, sizeof nm, "%s w=%u n=%llu frames=%u", name, c.tile_w, (unsigned long long)n_raw, n_frames);
    open("repair", nm, rc);
    num("path", P.path); num("n_tiles", P.n_tiles); num("blocks_per_tile", P.blocks_per_tile); num("in_bytes", P.in_bytes);
    num("f_n_frames", fp.n_frames); num("f_tiles_per_frame", fp.tiles_per_frame); num("f_one_launch", fp.one_launch); num("f_path", fp.path); num("f_in_bytes", fp.in_bytes); num("f_stride_min", fp.stride_min);
    printf("}");
}

}  // namespace

int main() {
    const int ks[4] = {24, 22, 20, 18};
    for (int i = 0; i < 4; ++i) kLutBytes[i] = synd_lut_bytes(ks[i]);
    const FusedForm forms[3] = {FusedForm::Words, FusedForm::Pixels, FusedForm::Rgb};
    const uint8_t kLuma[9] = {20, 22, 22, 20, 22, 22, 20, 22, 22}, kThree[9] = {18, 18, 18, 22, 22, 22, 24, 24, 24}, kFour[9] = {18, 18, 20, 20, 22, 22, 24, 24, 24};
    printf("[");
    // ---- fused: each k and form; a tile of k = 22 decodes 54 * 22 = 1188 words: frames of nothing, a word, either side of one and two tiles, 8K words
    for (int k : ks) for (FusedForm f : forms) { char nm[8]; snprintf(nm, sizeof nm, "k%d", k); fused(nm, cfg_k(k), 54ull * k + 3, f); }
    for (uint64_t n : {0ull, 1ull, 1186ull, 1190ull, 2375ull, 2378ull, 8192ull}) fused("k22", cfg_k(22), n, n % 2 ? FusedForm::Words : FusedForm::Pixels);
    // a beacon stepped over in the loads
    for (uint32_t period : {2u, 3u, 64u}) for (uint32_t slot : {0u, 8u}) fused("k20 beacon", with_beacon(cfg_k(20), period, slot), 8192, forms[(period + slot / 8) % 3], true);
    fused("k20 beacon stripped", with_beacon(cfg_k(20), 64, 2), 8192, FusedForm::Pixels);
    // tile ranges of a frame of seven tiles: first, last, inner, the whole range given, past the end, empty, reversed; forms and beacons that take none
    for (auto r : {std::pair<uint32_t, uint32_t>{0, 1}, {6, 7}, {6, 0xFFFFFFFFu}, {2, 5}, {1, 9}, {3, 3}, {5, 3}, {9, 12}}) fused("k22 range", cfg_k(22), 8192, FusedForm::Pixels, false, r.first, r.second);
    fused("k22 range", cfg_k(22), 8192, FusedForm::Rgb, false, 2, 5);
    fused("k22 range", cfg_k(22), 8192, FusedForm::Words, false, 1, 3);
    fused("k20 beacon range", with_beacon(cfg_k(20), 64, 2), 8192, FusedForm::Pixels, true, 1, 3);
    // not its framing: 2-D, several k
    fused("k22 2d", cfg_k(22, 64), 8192, FusedForm::Pixels); fused("luma", cfg_of(kLuma), 8192, FusedForm::Pixels);
    // the repair form: each k, 1-D and 2-D
    for (int k : ks) { char nm[8]; snprintf(nm, sizeof nm, "k%d", k); fused(nm, cfg_k(k), 8192, FusedForm::Repair); }
    fused("k22", cfg_k(22), 1, FusedForm::Repair); fused("k22", cfg_k(22, 64), 8192, FusedForm::Repair);
    // ---- UEP: the ten (ra, rb), either group first; 2-D widths; chunks below and above n_sym; what it refuses
    for (int i = 0; i < 4; ++i) for (int j = i; j < 4; ++j) for (int sw = 0; sw < (i == j ? 1 : 2); ++sw) {
        uint8_t k9[9]; for (int b = 0; b < 9; ++b) k9[b] = (uint8_t)((b % 3 == 0) != (sw != 0) ? ks[i] : ks[j]);
        char nm[24]; snprintf(nm, sizeof nm, "k%dk%d", k9[0], k9[1]);
        if (sw == 0 || j - i == 1) uep(nm, cfg_of(k9), 8192);
    }
    for (uint32_t w : {1u, 4u, 6u, 64u, 512u}) uep(w == 64 ? "k22" : "luma", w == 64 ? cfg_k(22, w) : cfg_of(kLuma, w), 8192);
    for (uint32_t h : {1u, 1200u}) uep("luma", cfg_of(kLuma, 64, h), 8192);           // n_sym = 70998: chunks of 64 and 76800
    uep("luma", cfg_of(kLuma, 4, 1), 8192); uep("luma", cfg_of(kLuma, 36, 3), 8192);       // a chunk of 108: no multiple of 16
    for (uint64_t n : {0ull, 1ull, 1100ull, 1200ull, 2300ull, 2500ull}) uep("luma", cfg_of(kLuma), n);
    uep("three k", cfg_of(kThree), 8192); uep("luma", cfg_of(kLuma), 8192, true); uep("luma", cfg_of(kLuma), 8192, false, 1ull << 28); uep("luma", cfg_of(kLuma), 8192, false, (1ull << 28) - 1);
    // ---- two kernels: one to four k, 1-D and 2-D with rows and chunks of whole granules (il_fast) or not, words and pixels
    for (int px = 0; px < 2; ++px) { stream("three k", cfg_of(kThree), 8192, px); stream("four k", cfg_of(kFour), 8192, px); stream("three k", cfg_of(kThree, 64, 64), 8192, px); stream("k22", cfg_k(22, 6, 64), 8192, px); }
    for (uint64_t n : {0ull, 1ull, 1000ull}) stream("three k", cfg_of(kThree), n, 0);
    stream("k24", cfg_k(24), 8192, 1); stream("luma", cfg_of(kLuma), 8192, 0);
    for (auto t : {std::pair<uint32_t, uint32_t>{64, 1200}, {48, 3}, {1, 1}, {16, 5}}) stream("three k", cfg_of(kThree, t.first, t.second), 8192, 0);
    // ---- window plans: the cases of tests/test_window_plan.py ...
    {
        const uint32_t fw = 7680, fh = 4320; const uint64_t n_raw = (uint64_t)fw * fh / 2;
        const uint32_t std_res[4][2] = {{3840, 2160}, {1920, 1080}, {1280, 720}, {854, 480}};
        for (int k : ks) {
            char nm[8]; snprintf(nm, sizeof nm, "k%d", k);
            for (auto& r : std_res) window(nm, cfg_k(k), n_raw, fw, fh, (fw - r[0]) / 2, (fh - r[1]) / 2, r[0], r[1]);
            const uint32_t wins[6][4] = {{0, 0, 1, 1}, {fw - 1, fh - 1, 1, 1}, {0, 100, fw, 7}, {0, 0, fw, fh}, {3, 5, 11, 1}, {100, fh - 10, 500, 50}};
            for (auto& q : wins) window(nm, cfg_k(k), n_raw, fw, fh, q[0], q[1], q[2], q[3]);
        }
        const uint32_t w2 = 960, h2 = 540; const uint64_t n2 = (uint64_t)w2 * h2 / 2; const t3_cfg c20 = cfg_k(20);
        window("k20", c20, n2, w2, h2, 0, h2, 10, 10); window("k20", c20, n2, w2, h2, 5, h2 + 7, 3, 1);
        window("k20", c20, n2 / 2, w2, h2, 0, h2 / 2 + 1, w2, 10); window("k20", c20, n2 / 2, w2, h2, 0, h2 / 2 - 3, w2, 10);
        window("k20", c20, n2, w2, h2, 0, 0, 0, 5); window("k20", c20, n2, w2, h2, 0, 0, 5, 0); window("k20", c20, n2, w2, h2, 0, 0, 0, 0);
        window("k20", c20, n2, w2, h2, w2 - 3, 0, 4, 1); window("k20", c20, n2, 0, h2, 0, 0, 0, 1); window("k20", c20, n2, w2, h2, 0xFFFFFFFFu, 0, 2, 1);
        { t3_cfg raw = c20; raw.profile = T3_RAW_MODE; window("raw", raw, n2, w2, h2, 0, 0, 4, 4); }
        window("luma", cfg_of(kLuma), n2, w2, h2, 10, 10, 100, 100); window("k20 2d", cfg_k(20, 64), n2, w2, h2, 10, 10, 100, 100); window("luma 2d", cfg_of(kLuma, 64), n2, w2, h2, 10, 10, 100, 100);
        window("k22 beacon", with_beacon(cfg_k(22), 83, 2), n2, w2, h2, 10, 10, 100, 100); window("k20 compat", cfg_k(20, 0, 0, T3_MODE_COMPAT), n2, w2, h2, 10, 10, 100, 100);
        { t3_cfg p5 = cfg_k(22); p5.profile = T3_P5_RS26_22_2D; window("k22 p5 1d", p5, n2, w2, h2, 10, 10, 100, 100); }
        window("k20", c20, n2, w2, h2, 10, 10, 100, 100, true); window("k20", c20, 0, w2, h2, 10, 10, 100, 100);
        // ... and of tests/test_frames_window_plan.py
        const uint32_t wins[9][6] = {{100, 70, 0, 0, 100, 70}, {100, 70, 10, 22, 50, 20}, {100, 70, 3, 44, 1, 1}, {100, 70, 37, 65, 63, 5}, {100, 80, 0, 60, 100, 20},
                                     {98, 72, 5, 1, 91, 3}, {100, 70, 0, 90, 10, 10}, {100, 70, 5, 5, 0, 9}, {100, 70, 5, 5, 9, 0}};
        for (auto& q : wins) { for (uint32_t n : {0u, 1u, 2u, 65535u}) frames_window("k24", cfg_k(24), 3500, n, q[0], q[1], q[2], q[3], q[4], q[5], 1); frames_window("k18", cfg_k(18), 3500, 3, q[0], q[1], q[2], q[3], q[4], q[5], 2); }
        for (auto& r : {std_res[0], std_res[3]}) frames_window("k22", cfg_k(22), n_raw, 4, fw, fh, (fw - r[0]) / 2, (fh - r[1]) / 2, r[0], r[1], 2);
        for (int fmt : {1, 2}) {
            frames_window("luma", cfg_of(kLuma), 3500, 3, 100, 70, 10, 22, 50, 20, fmt); frames_window("k22 2d", cfg_k(22, 64), 3500, 3, 100, 70, 10, 22, 50, 20, fmt);
            frames_window("k22 beacon", with_beacon(cfg_k(22), 83, 2), 3500, 3, 100, 70, 10, 22, 50, 20, fmt); frames_window("k20 compat", cfg_k(20, 0, 0, T3_MODE_COMPAT), 3500, 3, 100, 70, 10, 22, 50, 20, fmt);
        }
        { t3_cfg raw = c20; raw.profile = T3_RAW_MODE; frames_window("raw", raw, 3500, 3, 100, 70, 10, 22, 50, 20, 1); }
        frames_window("k20", c20, 3500, 3, 100, 70, 98, 0, 3, 1, 1); frames_window("k20", c20, 3500, 3, 0, 70, 0, 0, 0, 1, 1);
        frames_window("k20", c20, 3500, 3, 100, 70, 10, 22, 50, 20, 0); frames_window("k20", c20, 3500, 3, 100, 70, 10, 22, 50, 20, 3); frames_window("k20", c20, 3500, 65536, 100, 70, 10, 22, 50, 20, 1);
        frames_window("k20", c20, 3500, 3, 100, 70, 10, 22, 50, 20, 1, true);
        for (uint32_t tiles : {53687u, 53688u}) {     // 40,000 frames either side of 2^31 tickets
            const uint32_t n_px = 2 * (tiles * 52 * 20 * 9 * 3 / 26 - 40);
            frames_window("k20 tickets", c20, n_px / 2, 40000, n_px, 1, 0, 0, n_px, 1, 1); frames_window("k20 tickets", c20, n_px / 2, 40000, n_px, 1, 2160, 0, n_px - 2160, 1, 1);
            frames_window("k20 tickets", c20, n_px / 2, 1, n_px, 1, 0, 0, n_px, 1, 1);
        }
    }
    // ---- repair plans: each k, frame sizes, beacon, 2-D with rows of whole dwords or not, several k, what is refused
    for (int k : ks) { char nm[8]; snprintf(nm, sizeof nm, "k%d", k); for (uint64_t n : {0ull, 1ull, 54ull * k - 1, 54ull * k + 1, 8192ull}) repair(nm, cfg_k(k), n, 3); }
    for (uint32_t w : {4u, 6u, 64u, 513u}) repair("k22 2d", cfg_k(22, w), 8192, 2);
    for (uint32_t n : {0u, 1u, 2u, 65535u, 65536u}) repair("k22", cfg_k(22), 8192, n);
    repair("k22 beacon", with_beacon(cfg_k(22), 83, 2), 8192, 3); repair("luma", cfg_of(kLuma), 8192, 3); repair("four k 2d", cfg_of(kFour, 6), 8192, 3);
    repair("k20 compat", cfg_k(20, 0, 0, T3_MODE_COMPAT), 8192, 3); { t3_cfg raw = cfg_k(20); raw.profile = T3_RAW_MODE; repair("raw", raw, 8192, 3); }
    repair("k20 tickets", cfg_k(20), (uint64_t)(53688u * 52 * 20 * 9 * 3 / 26 - 40), 40000); repair("k20 tickets", cfg_k(20), (uint64_t)(53687u * 52 * 20 * 9 * 3 / 26 - 40), 40000);
    printf("]\n");
    fprintf(stderr, "%d cases\n", n_cases);
    return 0;
}
