// The closed-form corrector of RS(26,20) (csrc/t3_rs_solve3.h, the text the pixel kernels run) against the block decoder of
// csrc/t3_rs_core.h, on the host: every 2-error pattern, every 3-error pattern, and a seeded set of heavier rows (tests/test_fx3_closed_form.py
// reads the one JSON line this prints).  The code is linear, so a pattern is an error vector on the zero codeword.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <atomic>
#include <thread>
#include <vector>

#include "t3_host.hpp"
#include "t3_rs_solve3.h"

using namespace t3;

namespace {

// the field of fx2_solve on the host: the field's own tables, the root masks as t3_api_decode.cpp tabulates them
struct HostField {
    const RsTables* t; const uint32_t* root_tbl;
    uint32_t mad(uint32_t a, uint32_t x, uint32_t y) const { return t->add[a * 27u + t->mul[x * 27u + y]]; }
    uint32_t neg(uint32_t x) const { return t->neg[x]; }
    uint32_t inv(uint32_t x) const { return t->inv[x]; }
    uint32_t ninv(uint32_t x) const { return t->neg[t->inv[x]]; }
    uint32_t ex(uint32_t i) const { return t->exp[i]; }
    uint32_t roots(uint32_t i) const { return root_tbl[i]; }
};

std::vector<uint32_t> root_table(const RsTables& t) {
    std::vector<uint32_t> tbl(27 * 27 * 27);
    for (uint32_t idx = 0; idx < tbl.size(); ++idx) {
        const uint8_t sg[4] = {1, (uint8_t)(idx % 27), (uint8_t)(idx / 27 % 27), (uint8_t)(idx / 729)};
        uint32_t mask = 0;
        for (int i = 0; i < 26; ++i) {
            const uint8_t x = t.exp[i == 0 ? 0 : 26 - i];
            uint8_t acc = sg[3];
            for (int q = 2; q >= 0; --q) acc = t.add[t.mul[acc * 27 + x] * 27 + sg[q]];
            if (acc == 0) mask |= 1u << i;
        }
        tbl[idx] = mask;
    }
    return tbl;
}

struct Tally {
    uint64_t n = 0, fallback = 0, mismatch = 0, accepted = 0, refused = 0;
    void add(const Tally& o) { n += o.n; fallback += o.fallback; mismatch += o.mismatch; accepted += o.accepted; refused += o.refused; }
};

// One received row.  want_np > 0: the row is the zero codeword with exactly these want_np errors -- the closed form must decide it.
void one_row(const HostField& f, const RsView& g, const uint8_t* row, int want_np, Tally& ty) {
    uint8_t ref[26], S8[6];
    memcpy(ref, row, 26);
    const bool ref_ok = rs_decode_block<6>(g, ref, true);
    ++ty.n;
    if (rs_syndromes<6>(g, row, S8)) { ty.mismatch += want_np > 0; return; }           // a codeword never reaches the queue
    uint32_t S[6];
    for (int j = 0; j < 6; ++j) S[j] = S8[j];
    const Solve3 r = fx2_solve<6>(f, S);
    if (r.np == 0) { ++ty.fallback; return; }                                          // the kernel runs Berlekamp-Massey: the block decoder's own answer
    ++(ref_ok ? ty.accepted : ty.refused);
    uint8_t got[26];
    memcpy(got, row, 26);
    bool same = ref_ok && (want_np == 0 || (int)r.np == want_np);
    for (uint32_t e = 0; e < r.np; ++e) {
        if (r.pos[e] >= 26u || (e > 0 && r.pos[e] <= r.pos[e - 1]) || r.mag[e] == 0u) same = false;      // ascending positions, no empty correction
        else got[r.pos[e]] = g.S(got[r.pos[e]], (uint8_t)r.mag[e]);
    }
    if (!same || memcmp(got, ref, 26) != 0) ++ty.mismatch;
}

uint64_t lcg(uint64_t& s) { s = s * 6364136223846793005ull + 1442695040888963407ull; return s >> 33; }

}  // namespace

int main() {
    const Field& F = field();
    const RsView g = rs_view(F.t);
    const std::vector<uint32_t> rt = root_table(F.t);
    const HostField f{&F.t, rt.data()};

    // every pair: 325 position pairs x 26^2 magnitudes
    Tally two;
    for (int p0 = 0; p0 < 26; ++p0) for (int p1 = p0 + 1; p1 < 26; ++p1)
        for (int m0 = 1; m0 < 27; ++m0) for (int m1 = 1; m1 < 27; ++m1) {
            uint8_t row[26] = {0}; row[p0] = (uint8_t)m0; row[p1] = (uint8_t)m1;
            one_row(f, g, row, 2, two);
        }

    // every triple: 2,600 position triples x 26^3 magnitudes, the triples dealt out to a few threads
    std::vector<int> trip;
    for (int p0 = 0; p0 < 26; ++p0) for (int p1 = p0 + 1; p1 < 26; ++p1) for (int p2 = p1 + 1; p2 < 26; ++p2) trip.push_back(p0 | p1 << 8 | p2 << 16);
    unsigned nthr = std::thread::hardware_concurrency();
    nthr = nthr == 0 ? 1 : nthr > 8 ? 8 : nthr;
    std::vector<Tally> part(nthr);
    std::atomic<size_t> next{0};
    std::vector<std::thread> pool;
    for (unsigned w = 0; w < nthr; ++w) pool.emplace_back([&, w] {
        for (size_t i; (i = next.fetch_add(1)) < trip.size();) {
            const int p0 = trip[i] & 255, p1 = (trip[i] >> 8) & 255, p2 = trip[i] >> 16;
            for (int m0 = 1; m0 < 27; ++m0) for (int m1 = 1; m1 < 27; ++m1) for (int m2 = 1; m2 < 27; ++m2) {
                uint8_t row[26] = {0}; row[p0] = (uint8_t)m0; row[p1] = (uint8_t)m1; row[p2] = (uint8_t)m2;
                one_row(f, g, row, 3, part[w]);
            }
        }
    });
    for (auto& t : pool) t.join();
    Tally three;
    for (const Tally& p : part) three.add(p);

    // beyond t: 100,000 rows each with 4, 5 and 6 errors, and 100,000 random rows (seeded)
    Tally heavy[4];
    uint64_t seed = 0x7e57f3ull;
    for (int kind = 0; kind < 4; ++kind)
        for (int it = 0; it < 100000; ++it) {
            uint8_t row[26] = {0};
            if (kind == 3) for (int i = 0; i < 26; ++i) row[i] = (uint8_t)(lcg(seed) % 27);
            else for (int placed = 0; placed < 4 + kind;) { const int p = (int)(lcg(seed) % 26); if (row[p] == 0) { row[p] = (uint8_t)(1 + lcg(seed) % 26); ++placed; } }
            one_row(f, g, row, 0, heavy[kind]);
        }

    auto put = [](const char* name, const Tally& t, const char* end) {
        printf("\"%s\": {\"n\": %llu, \"fallback\": %llu, \"mismatch\": %llu, \"accepted\": %llu, \"refused\": %llu}%s", name, (unsigned long long)t.n, (unsigned long long)t.fallback,
               (unsigned long long)t.mismatch, (unsigned long long)t.accepted, (unsigned long long)t.refused, end);
    };
    printf("{");
    put("two", two, ", "); put("three", three, ", "); put("four", heavy[0], ", "); put("five", heavy[1], ", "); put("six", heavy[2], ", "); put("random", heavy[3], "}\n");
    return 0;
}
