// tests/cpp/frame_batch_demo.cpp — the host-side batch rules of the synchronous repair and erasure-decode entries (csrc/t3_frame_batch.hpp)
// on a fixed list of cases, without a device and without libt3hip.so: built by tests/test_frame_batch.py from this file, t3_frame_batch.cpp,
// t3_dec_plan.cpp and t3_host.cpp with plain g++.  A batch is a string, one letter a frame: 'A' / 'B' two configurations that differ only
// in their scrambler seeds, 'a' / 'b' the same with the second n_raw_words; behind a letter '-' damages the header within t (2 symbols of
// its first RS(26,18) block), '!' beyond it (9).  Each batch goes through the steps of t3hip_repair_frames_dev (plain, four words) and of
// t3hip_decode_erasures_frames_dev (pixels) as those entries call the unit, on verdict words the demo makes up, and one JSON record per
// batch and flow says what came out.  tests/test_frame_batch.py compares every field with a model of its own.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "t3_dec_plan.hpp"
#include "t3_frame_batch.hpp"

using namespace t3;

namespace {
const uint64_t kNRaw[2] = {64, 200};

t3_cfg cfg_of(bool second) {
    t3_cfg c; memset(&c, 0, sizeof c);
    c.profile = T3_P3_RS26_20; c.mode = T3_MODE_FIXED;
    for (int b = 0; b < 9; ++b) c.band_profile[b] = (uint8_t)k_index(20);
    c.seed_a = second ? 2 : 1; c.seed_b = second ? 5 : 1; c.seed_s0 = 1; c.superframe_words = 8192; c.subword = 27; c.centered = 1;
    return c;
}
struct Frame { bool second, big; int damage; };
std::vector<Frame> frames_of(const char* spec) {
    std::vector<Frame> fr;
    for (const char* p = spec; *p; ++p) {
        if (*p == '-') fr.back().damage = 2;
        else if (*p == '!') fr.back().damage = 9;
        else fr.push_back(Frame{*p == 'B' || *p == 'b', *p == 'a' || *p == 'b', 0});
    }
    return fr;
}
std::vector<uint8_t> headers_of(const std::vector<Frame>& fr) {
    std::vector<uint8_t> got(90 * fr.size());
    for (size_t f = 0; f < fr.size(); ++f) {
        uint8_t* h = &got[90 * f];
        header_encode(cfg_of(fr[f].second), kNRaw[fr[f].big], h);
        for (int i = 0; i < fr[f].damage; ++i) h[2 * i + 1] = (uint8_t)((h[2 * i + 1] + 1 + i % 25) % 27);
    }
    return got;
}
t3_cfg seen0() { t3_cfg c; memset(&c, 0, sizeof c); c.mode = T3_MODE_FIXED; return c; }
uint32_t word(uint32_t f, uint32_t i) { return i == 1 ? f % 3 == 2 : 100 * f + i; }      // the made-up verdict words: every third frame fails

template <class T> void arr(const char* name, const T* v, size_t n) {
    printf(",\"%s\":[", name);
    for (size_t i = 0; i < n; ++i) printf("%s%lld", i ? "," : "", (long long)v[i]);
    printf("]");
}
int n_records = 0;
void open(const char* kind, const char* name) { printf("%s{\"kind\":\"%s\",\"case\":\"%s\"", n_records++ ? ",\n" : "", kind, name); }
void seen_out(const t3_cfg& s, const std::vector<FrameHeader>& hd) {      // the first frame that counts and whose parsed configuration `seen` is
    int of = -1;
    for (size_t f = 0; f < hd.size() && of < 0; ++f) if (hd[f].ok && memcmp(&hd[f].cfg, &s, sizeof s) == 0) of = (int)f;
    printf(",\"seen_profile\":%d,\"seen_mode\":%d,\"seen_frame\":%d", (int)s.profile, (int)s.mode, of);
}
void runs_out(const std::vector<uint8_t>& go, const std::vector<FrameHeader>& hd) {
    printf(",\"runs\":[");
    int n = 0;
    for (uint32_t f0 = 0, f1 = 0; next_run(go.data(), hd.data(), (uint32_t)go.size(), f1, &f0, &f1);) printf("%s[%u,%u]", n++ ? "," : "", f0, f1);
    printf("]");
}
void fold_out(uint32_t nw, const std::vector<uint8_t>& go, std::vector<uint32_t>& counts, std::vector<int>& rcs) {
    const uint32_t N = (uint32_t)go.size();
    std::vector<uint32_t> v(nw * N);
    for (uint32_t f = 0; f < N; ++f) for (uint32_t i = 0; i < nw; ++i) v[nw * f + i] = go[f] ? word(f, i) : 0xDEADu;      // (never read where the frame did not run)
    fold_verdicts(v.data(), nw, N, go.data(), counts.data(), rcs.data());
    arr("counts", counts.data(), counts.size()); arr("frame_rc", rcs.data(), rcs.size());
}

// t3hip_repair_frames_dev behind its argument checks
void repair_flow(const char* spec, uint64_t n_in) {
    const std::vector<Frame> fr = frames_of(spec); const uint32_t N = (uint32_t)fr.size(), nw = 4;
    const std::vector<uint8_t> got = headers_of(fr);
    std::vector<uint8_t> fix(90 * N), differs(N), go(N);
    std::vector<FrameHeader> hd(N); std::vector<t3_repair_plan> P(N); std::vector<t3_layout> L(N);
    std::vector<uint32_t> counts(nw * N, 0); std::vector<int> rcs(N, T3_E_HEADER);
    t3_cfg seen = seen0();
    const bool any = parse_headers(got.data(), N, n_in, &seen, hd.data(), L.data(), go.data(), [&](uint32_t f, uint64_t n_raw, const t3_cfg& cfg, t3_layout& l) {
        return header_codewords(&got[90 * f], &fix[90 * f], &differs[f]) ? plan_repair(n_raw, cfg, P[f], l) : T3_E_HEADER; });
    char nm[96]; snprintf(nm, sizeof nm, "%s n_in=%llu", spec, (unsigned long long)n_in);
    open("repair", nm);
    printf(",\"rc\":%d", any ? T3_OK : T3_E_HEADER);
    std::vector<int> ok(N), nraw(N), next_ok(N), fixed_ok(N);
    for (uint32_t f = 0; f < N; ++f) {
        ok[f] = hd[f].ok; nraw[f] = hd[f].ok ? (int)hd[f].n_raw : -1;
        const KnownFrame k = known_frame(cfg_of(fr[f].second), kNRaw[fr[f].big]);
        next_ok[f] = hd[f].ok && memcmp(hd[f].next, k.next, 3) == 0;                // the parsed table is the configuration's
        fixed_ok[f] = hd[f].ok && k.hs == 90 && memcmp(&fix[90 * f], k.hx.b, 90) == 0;   // the codewords are the bytes the configuration encodes to
    }
    arr("ok", ok.data(), N); arr("n_raw", nraw.data(), N); arr("next_ok", next_ok.data(), N); arr("fixed_ok", fixed_ok.data(), N);
    if (any) {
        seen_out(seen, hd); runs_out(go, hd);
        for (uint32_t f = 0; f < N; ++f) if (go[f]) counts[nw * f] = differs[f];
        fold_out(nw, go, counts, rcs);
    }
    printf("}");
}

// t3hip_decode_erasures_frames_dev (pixels) behind its argument checks
void decode_flow(const char* spec, uint64_t n_in, uint64_t cap_units) {
    const std::vector<Frame> fr = frames_of(spec); const uint32_t N = (uint32_t)fr.size();
    const std::vector<uint8_t> got = headers_of(fr);
    std::vector<uint8_t> go(N);
    std::vector<FrameHeader> hd(N); std::vector<t3_decode_erasures_plan> P(N); std::vector<t3_layout> L(N); std::vector<uint64_t> units(N);
    std::vector<uint32_t> counts(4 * N, 0); std::vector<int> rcs(N, T3_E_HEADER);
    t3_cfg seen = seen0();
    const bool any = parse_headers(got.data(), N, n_in, &seen, hd.data(), L.data(), go.data(), [&](uint32_t f, uint64_t n_raw, const t3_cfg& cfg, t3_layout& l) {
        const int rc = plan_decode_erasures(n_raw, cfg, 1, P[f], l); units[f] = P[f].out_units; return rc; });
    char nm[96]; snprintf(nm, sizeof nm, "%s n_in=%llu cap=%llu", spec, (unsigned long long)n_in, (unsigned long long)cap_units);
    open("decode", nm);
    printf(",\"rc\":%d", any ? T3_OK : T3_E_HEADER);
    std::vector<int> ok(N);
    for (uint32_t f = 0; f < N; ++f) ok[f] = hd[f].ok;
    arr("ok", ok.data(), N);
    if (any) {
        const uint64_t n_out = select_equal_frames(units.data(), N, cap_units, go.data(), rcs.data());
        printf(",\"n_out\":%llu", (unsigned long long)n_out);
        arr("go", go.data(), N); seen_out(seen, hd); runs_out(go, hd); fold_out(4, go, counts, rcs);
    }
    printf("}");
}
}  // namespace

int main() {
    printf("[");
    // what the model is told about the two sizes and the two configurations
    open("facts", "facts");
    for (int big = 0; big < 2; ++big) {
        t3_repair_plan P; t3_layout L; t3_decode_erasures_plan D; t3_layout L2;
        const int rc = plan_repair(kNRaw[big], cfg_of(false), P, L) | plan_decode_erasures(kNRaw[big], cfg_of(false), 1, D, L2);
        printf(",\"rc%d\":%d,\"n_raw%d\":%llu,\"out_words%d\":%llu,\"units%d\":%llu", big, rc, big, (unsigned long long)kNRaw[big], big, (unsigned long long)L.out_words, big, (unsigned long long)D.out_units);
    }
    const KnownFrame ka = known_frame(cfg_of(false), kNRaw[0]), kb = known_frame(cfg_of(true), kNRaw[0]);
    arr("next_a", ka.next, 3); arr("next_b", kb.next, 3);
    printf(",\"hs\":%u,\"headers_differ\":%d}", ka.hs, memcmp(ka.hx.b, kb.hx.b, 96) != 0);
    const uint64_t w0 = [] { t3_repair_plan P; t3_layout L; plan_repair(kNRaw[0], cfg_of(false), P, L); return L.out_words; }();
    const uint64_t w1 = [] { t3_repair_plan P; t3_layout L; plan_repair(kNRaw[1], cfg_of(false), P, L); return L.out_words; }();
    const uint64_t u0 = 2 * kNRaw[0];
    const char* const specs[] = {"AAAA", "A!AAA", "AA!AA", "AAA!", "A!A!A!", "AABBA", "AAa", "aAA", "A-AB-B!A", "A", "A!", "A-", "AB", "AA", "A!A", "AbaB"};
    for (const char* s : specs) {
        repair_flow(s, w1);
        decode_flow(s, w1, 2 * kNRaw[1]);
    }
    decode_flow("AAAA", w1, u0 - 1); decode_flow("A!AaA", w1, u0 - 1); decode_flow("aAA", w1, u0);       // capacity one short; the big frames one short
    repair_flow("AAaA", w0); decode_flow("AAaA", w0, 2 * kNRaw[1]); repair_flow("aAA", w1 - 1); decode_flow("aaA", w1 - 1, 2 * kNRaw[1]);   // truncated by n_in
    repair_flow("AA", 9); repair_flow("aa", w0);                                    // no room for a header; every frame truncated

    // the single-frame acceptance: what plan_of gives passes through as it is (the entries map it where they call)
    {
        const std::vector<uint8_t> good = headers_of(frames_of("A")), bad = headers_of(frames_of("A!"));
        FrameHeader h; t3_layout L; t3_repair_plan P;
        auto plan_of = [&](uint64_t n_raw, const t3_cfg& cfg, t3_layout& l) { return plan_repair(n_raw, cfg, P, l); };
        open("accept", "single");
        printf(",\"good\":%d", accept_header(good.data(), w0, seen0(), h, L, plan_of)); printf(",\"good_ok\":%d", h.ok);
        printf(",\"beyond_t\":%d", accept_header(bad.data(), w0, seen0(), h, L, plan_of)); printf(",\"beyond_t_ok\":%d", h.ok);
        printf(",\"truncated\":%d", accept_header(good.data(), w0 - 1, seen0(), h, L, plan_of)); printf(",\"truncated_ok\":%d", h.ok);
        printf(",\"plan_arg\":%d", accept_header(good.data(), w0, seen0(), h, L, [](uint64_t, const t3_cfg&, t3_layout&) { return T3_E_ARG; })); printf(",\"plan_arg_ok\":%d", h.ok);
        printf(",\"plan_other\":%d", accept_header(good.data(), w0, seen0(), h, L, [](uint64_t, const t3_cfg&, t3_layout&) { return T3_E_CAPACITY; }));
        uint8_t fix[90], differs = 7; const std::vector<uint8_t> within = headers_of(frames_of("A-"));
        printf(",\"codewords_clean\":%d", header_codewords(good.data(), fix, &differs)); printf(",\"differs_clean\":%d", differs);
        printf(",\"codewords_within\":%d", header_codewords(within.data(), fix, &differs)); printf(",\"differs_within\":%d,\"fixed\":%d", differs, memcmp(fix, good.data(), 90) == 0);
        printf(",\"codewords_beyond\":%d}", header_codewords(bad.data(), fix, &differs));
    }

    // the address rule: [base, n_in, stride, n_frames] -> ok
    {
        const uint64_t edge = (~0ull) / 9;
        const uint64_t q[][4] = {{64, 100, 900, 3}, {65, 100, 900, 3}, {64, 100, 901, 3}, {64, 100, 898, 3}, {64, 100, 902, 3}, {64, 101, 910, 2}, {64, 101, 909, 2}, {64, 101, 908, 2},
                                 {64, 100, 0, 1}, {64, 100, 1, 1}, {65, 100, 900, 1}, {64, 100, 0, 0}, {64, 0, 0, 2}, {0, 0, 0, 2}, {64, edge, 0, 1}, {64, edge + 1, 0, 1},
                                 {64, edge, 9 * edge - 1, 2}, {64, edge - 1, 9 * (edge - 1), 2}, {64, edge + 1, ~0ull - 1, 2}};
        open("address", "rule");
        printf(",\"cases\":[");
        for (size_t i = 0; i < sizeof q / sizeof q[0]; ++i)
            printf("%s[%llu,%llu,%llu,%llu,%d]", i ? "," : "", (unsigned long long)q[i][0], (unsigned long long)q[i][1], (unsigned long long)q[i][2], (unsigned long long)q[i][3],
                   batch_in_ok((const void*)(uintptr_t)q[i][0], q[i][1], q[i][2], (uint32_t)q[i][3]) ? 1 : 0);
        printf("]}");
    }
    // the staging geometry: [n_in, stride, n_frames] -> bytes, dev_stride, pitch
    {
        const uint64_t q[][3] = {{100, 1000, 3}, {101, 1000, 3}, {101, 909, 2}, {100, 1000, 1}, {101, 5, 1}, {0, 0, 2}, {1, 9, 2}};
        open("stage", "geometry");
        printf(",\"cases\":[");
        for (size_t i = 0; i < sizeof q / sizeof q[0]; ++i) {
            const FrameStage g = frame_stage(q[i][0], q[i][1], (uint32_t)q[i][2]);
            printf("%s[%llu,%llu,%llu,%llu,%llu,%llu]", i ? "," : "", (unsigned long long)q[i][0], (unsigned long long)q[i][1], (unsigned long long)q[i][2],
                   (unsigned long long)g.bytes, (unsigned long long)g.dev_stride, (unsigned long long)g.pitch);
        }
        printf("]}");
    }
    printf("]\n");
    return 0;
}
