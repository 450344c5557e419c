// tests/cpp/stage_names_demo.cpp — the reference decoder's stage functions (read_and_decode_header_from_words,
// descramble_words_inplace, demap_and_rsdecode_bands_from_words: OLD:918-993) and its single-word subword helpers
// (extract_subword_trits_from_word, inject_subword_trits_into_word: OLD:816-833) called by their reference names through
// include/compat.  tests/test_decode_stages.py writes the inputs as files and checks the JSON line against the oracle.
//   stage_names_demo host CASES      word helpers and header reads (host arithmetic: no device needed)
//   stage_names_demo dev STREAM...   decode_profile_to_raw spelled out from the stages (OLD:995-1041) next to the drop-in's own
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "ternary_image_codec_v6_min.hpp"   // include/compat

static uint64_t fnv(const void* p, size_t n) { const uint8_t* b = (const uint8_t*)p; uint64_t h = 1469598103934665603ull; for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 1099511628211ull; } return h; }

static std::vector<uint8_t> slurp(const char* path) {
    std::vector<uint8_t> d; FILE* f = std::fopen(path, "rb"); if (!f) return d;
    uint8_t buf[65536]; size_t n;
    while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) d.insert(d.end(), buf, buf + n);
    std::fclose(f); return d;
}
struct Reader {
    const std::vector<uint8_t>& d; size_t p = 0;
    template <class T> T get() { T v; std::memcpy(&v, d.data() + p, sizeof v); p += sizeof v; return v; }
};
static void print_u8(const uint8_t* p, size_t n) { std::printf("["); for (size_t i = 0; i < n; ++i) std::printf(i ? ",%d" : "%d", p[i]); std::printf("]"); }

// decode_profile_to_raw, statement for statement as OLD:995-1041, on the drop-in's stage functions
static bool spelled_decode(const std::vector<Word27>& in, std::vector<Word27>& out, DecoderContext& dctx) {
    out.clear();
    if (dctx.cfg_last_seen.profile == ProfileID::RAW_MODE) { out = in; return true; }
    size_t cur = 0;
    SuperframeHeader hdr{};
    if (!read_and_decode_header_from_words(in, cur, hdr, dctx.rs_hdr)) return false;
    dctx.cfg_last_seen.profile = hdr.profile;
    dctx.cfg_last_seen.uep = hdr.uep;
    dctx.cfg_last_seen.tile = hdr.tile;
    dctx.cfg_last_seen.seed = hdr.seed;
    dctx.cfg_last_seen.beacon = hdr.beacon;
    dctx.cfg_last_seen.subword = hdr.subword;
    dctx.cfg_last_seen.centered = hdr.centered;
    dctx.cfg_last_seen.coset = hdr.coset;
    std::vector<Word27> body(in.begin() + (std::ptrdiff_t)cur, in.end());
    descramble_words_inplace(body, hdr);
    std::vector<GF27> use;
    if (!demap_and_rsdecode_bands_from_words(body, use, hdr, dctx.rs_p1, dctx.rs_p2, dctx.rs_p3, dctx.rs_p4)) return false;
    if (hdr.profile == ProfileID::P5_RS26_22_2D && hdr.tile.w && hdr.tile.h) deinterleave2D_boustrophedon(use, hdr.tile);
    std::vector<UTrit> tr;
    tr.reserve(use.size() * 3);
    for (auto s : use) { auto d = unpack3(s); tr.insert(tr.end(), d.begin(), d.end()); }
    size_t idx = 0;
    while (idx + 26 <= tr.size()) {
        std::array<UTrit, 27> T{};
        for (int i = 0; i < 26; ++i) T[(size_t)i] = tr[idx + (size_t)i];
        T[26] = 0;
        Word27 w{};
        for (int s = 0; s < 9; ++s) w.sym[(size_t)s] = pack3(T[(size_t)(s * 3)], T[(size_t)(s * 3 + 1)], T[(size_t)(s * 3 + 2)]);
        out.push_back(w);
        idx += 26;
    }
    return true;
}
static void print_seen(const DecoderConfigSeen& c) {
    std::printf("{\"profile\":%d,\"band_profile\":", (int)c.profile); print_u8(c.uep.band_profile.data(), 9);
    std::printf(",\"tile_w\":%d,\"tile_h\":%d,\"seed_a\":%u,\"seed_b\":%u,\"seed_s0\":%u,\"beacon_words_period\":%u,\"beacon_band_slot\":%d,\"beacon_enabled\":%d,"
                "\"subword\":%d,\"centered\":%d,\"coset\":%d}", c.tile.w, c.tile.h, c.seed.a, c.seed.b, c.seed.s0, c.beacon.words_period, c.beacon.band_slot,
                c.beacon.enabled ? 1 : 0, (int)c.subword, c.centered ? 1 : 0, (int)c.coset);
}

int main(int argc, char** argv) {
    if (argc >= 3 && std::string(argv[1]) == "host") {
        // CASES: u32 n, n words (extract); u32 n, n x {i32 N, u8 fill, 30 trits} (inject); u32 n, n x {u32 words, u64 cursor, u8 mode, 9 words bytes}
        const std::vector<uint8_t> d = slurp(argv[2]); Reader r{d};
        std::printf("{\"extract\":[");
        const uint32_t ne = r.get<uint32_t>();
        for (uint32_t i = 0; i < ne; ++i) {
            Word27 w; std::memcpy(w.sym.data(), d.data() + r.p, 9); r.p += 9;
            std::array<UTrit, 27> T; T.fill(99);
            extract_subword_trits_from_word(w, (int)(i % 28), T);
            if (i) std::printf(","); print_u8(T.data(), 27);
        }
        std::printf("],\"inject\":[");
        const uint32_t ni = r.get<uint32_t>();
        for (uint32_t i = 0; i < ni; ++i) {
            const int N = r.get<int32_t>(); const UTrit fill = r.get<uint8_t>();
            UTrit in[30]; std::memcpy(in, d.data() + r.p, 30); r.p += 30;
            Word27 w; w.sym.fill(99);
            if (fill == 0 && (i & 1)) inject_subword_trits_into_word(in, N, w);     // the default argument
            else inject_subword_trits_into_word(in, N, w, fill);
            if (i) std::printf(","); print_u8(w.sym.data(), 9);
        }
        std::printf("],\"header\":[");
        const uint32_t nh = r.get<uint32_t>();
        for (uint32_t i = 0; i < nh; ++i) {
            const uint32_t nw = r.get<uint32_t>(); size_t cursor = (size_t)r.get<uint64_t>(); const uint8_t mode = r.get<uint8_t>();
            std::vector<Word27> words(nw); if (nw) std::memcpy(words.data(), d.data() + r.p, 9 * (size_t)nw); r.p += 9 * (size_t)nw;
            DecoderContext dctx; dctx.cfg_last_seen.mode = mode;
            SuperframeHeader h; h.frame_seq = 4242;                          // untouched unless the call succeeds
            const bool ok = read_and_decode_header_from_words(words, cursor, h, dctx.rs_hdr);
            DecoderConfigSeen s; s.profile = h.profile; s.uep = h.uep; s.tile = h.tile; s.seed = h.seed; s.beacon = h.beacon; s.subword = h.subword;
            s.centered = h.centered; s.coset = h.coset;
            std::printf("%s{\"ok\":%d,\"cursor\":%zu,\"frame_seq\":%u,\"band_map_hash\":%u,\"magic\":%u,\"version\":%u,\"hdr\":", i ? "," : "", ok ? 1 : 0, cursor,
                        h.frame_seq, h.band_map_hash, h.magic, h.version);
            print_seen(s); std::printf("}");
        }
        std::printf("]}\n");
        return 0;
    }
    if (argc >= 3 && std::string(argv[1]) == "dev") {
        std::printf("{\"status\":%d,\"streams\":[", t3::ensure_device() ? 0 : t3::last_status());
        for (int a = 2; a < argc; ++a) {
            const std::vector<uint8_t> d = slurp(argv[a]);
            std::vector<Word27> in(d.size() / 9); if (!in.empty()) std::memcpy(in.data(), d.data(), 9 * in.size());
            DecoderContext d1, d2; std::vector<Word27> o1, o2;
            const bool ok1 = spelled_decode(in, o1, d1), ok2 = decode_profile_to_raw(in, o2, d2);
            std::printf("%s{\"ok_spelled\":%d,\"ok_dropin\":%d,\"n_spelled\":%zu,\"n_dropin\":%zu,\"h_spelled\":\"%016llx\",\"h_dropin\":\"%016llx\",\"seen_spelled\":",
                        a > 2 ? "," : "", ok1 ? 1 : 0, ok2 ? 1 : 0, o1.size(), o2.size(), (unsigned long long)fnv(o1.data(), 9 * o1.size()),
                        (unsigned long long)fnv(o2.data(), 9 * o2.size()));
            print_seen(d1.cfg_last_seen); std::printf(",\"seen_dropin\":"); print_seen(d2.cfg_last_seen); std::printf("}");
        }
        std::printf("]}\n");
        return 0;
    }
    std::fprintf(stderr, "usage: %s host CASES | dev STREAM...\n", argv[0]);
    return 2;
}
