// synd_operand3.cpp — host model of the three-step syndrome operand of the fused FIXED decoders (csrc/t3_decode_fx2.h, fx2_set).
// A lane holds 13 symbols as 4-byte T entries (trit0 | trit1 << 8 | descrambled symbol << 16 | trit2 << 24); twelve of them fill the
// three K-steps of v_mfma_i32_32x32x32_i8, and the trits of the 13th ride in byte 2 of step 0's dwords 0, 1, 2, where
// build_mfma_syndrome (csrc/t3_host.cpp) has their coefficients -- every other byte 2 of the A operand is zero, so the descrambled
// symbols that stay in the other byte-2 places count for nothing.
// The program builds the B bytes as the kernel does, forms the 32 rows' integer dot products with the A operand, folds them mod 3 and
// compares with rs_syndromes (csrc/t3_rs_core.h) of the descrambled block, for k = 24, 22, 20, 18:
//   single   every position 0..25 x symbol value 0..26 x scrambler state 0..2 on an otherwise zero block
//   random   100,000 seeded blocks of random coded symbols and states
// and checks that every partial sum stays in [-78, 78].  One JSON line of tallies; exit status 1 on any mismatch.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "t3_host.hpp"
#include "t3_rs_core.h"

using namespace t3;

namespace {

// v_perm_b32: byte i of the result is picked by byte i of sel -- 0..3 from s1, 4..7 from s0
uint32_t perm(uint32_t s0, uint32_t s1, uint32_t sel) {
    const uint64_t src = (uint64_t)s0 << 32 | s1;
    uint32_t r = 0;
    for (int i = 0; i < 4; ++i) r |= (uint32_t)((src >> (8 * ((sel >> (8 * i)) & 7u))) & 0xFFu) << (8 * i);
    return r;
}

struct Tally { long n = 0, mismatch = 0, out_of_range = 0; };

std::vector<uint32_t> T;          // build_syndrome_T, one copy: entry 27 state + coded symbol

// coded[26], state[26] -> the block as the kernel sees it.  Returns false on a mismatch.
template <int R>
void check_block(const std::vector<uint32_t>& A, const uint8_t* coded, const uint8_t* state, Tally& t) {
    const Field& F = field(); const RsView v = rs_view(F.t);
    constexpr int H = R / 2;
    uint32_t B[3][2][4];                                                          // [step][lane half][dword]
    uint8_t desc[26];
    for (int h = 0; h < 2; ++h) {
        uint32_t E[13];
        for (int q = 0; q < 13; ++q) {
            const int p = 13 * h + q;
            E[q] = T[27 * state[p] + coded[p]];
            desc[p] = F.t.add[coded[p] * 27 + F.t.neg[13 * state[p]]];            // descramble_symbol, independently of T
            if (((E[q] >> 16) & 0xFFu) != desc[p]) ++t.mismatch;
        }
        for (int st = 0; st < 3; ++st) for (int d = 0; d < 4; ++d) B[st][h][d] = E[4 * st + d];
        B[0][h][0] = perm(E[12], B[0][h][0], 0x03040100u);                          // the spare-byte insertion of fx2_set
        B[0][h][1] = perm(E[12], B[0][h][1], 0x03050100u);
        B[0][h][2] = perm(E[12], B[0][h][2], 0x03070100u);
    }
    uint8_t S[R]; rs_syndromes<R>(v, desc, S);
    int got[R]; for (int j = 0; j < R; ++j) got[j] = 0;
    for (int m = 0; m < 32; ++m) {
        int acc = 0; bool in_range = true;
        for (int st = 0; st < 3; ++st) for (int h = 0; h < 2; ++h) for (int d = 0; d < 4; ++d) for (int b = 0; b < 4; ++b) {
            acc += (int)(int8_t)(A[(size_t)(st * 64 + 32 * h + m) * 4 + d] >> (8 * b)) * (int)(int8_t)(B[st][h][d] >> (8 * b));
            in_range = in_range && acc >= -78 && acc <= 78;
        }
        if (!in_range) ++t.out_of_range;
        const int i = (m & 3) + 4 * (m >> 3), hh = (m >> 2) & 1;
        const int trit = ((acc % 3) + 3) % 3;
        if (i < 3 * H) got[hh * H + i / 3] += trit * (i % 3 == 0 ? 1 : i % 3 == 1 ? 3 : 9);
        else if (acc != 0) ++t.mismatch;                                           // rows without a syndrome trit are zero rows
    }
    ++t.n;
    for (int j = 0; j < R; ++j) if (got[j] != S[j]) { ++t.mismatch; break; }
}

template <int R>
void run(Tally& single, Tally& random) {
    std::vector<uint32_t> A; build_mfma_syndrome(26 - R, A);
    if (A.size() != 3u * 64u * 4u) { ++single.mismatch; return; }
    // byte 2 is zero everywhere but in dwords 0, 1, 2 of step 0
    for (size_t i = 0; i < A.size(); ++i) if (((A[i] >> 16) & 0xFFu) != 0u && !(i < 64u * 4u && (i & 3u) < 3u)) ++single.mismatch;
    const Field& F = field();
    uint8_t coded[26], state[26];
    for (int p = 0; p < 26; ++p) for (int val = 0; val < 27; ++val) for (int s = 0; s < 3; ++s) {
        for (int i = 0; i < 26; ++i) { state[i] = (uint8_t)s; coded[i] = F.t.add[0 * 27 + 13 * s]; }   // the zero symbol, scrambled
        coded[p] = F.t.add[val * 27 + 13 * s];
        check_block<R>(A, coded, state, single);
    }
    uint64_t x = 0x9E3779B97F4A7C15ull + (uint64_t)R;
    auto rnd = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return (uint32_t)(x >> 33); };
    for (int n = 0; n < 100000; ++n) {
        for (int i = 0; i < 26; ++i) { coded[i] = (uint8_t)(rnd() % 27u); state[i] = (uint8_t)(rnd() % 3u); }
        check_block<R>(A, coded, state, random);
    }
}

}  // namespace

int main() {
    build_syndrome_T(T, 1);
    bool ok = true;
    printf("{");
    for (int ki = 0; ki < 4; ++ki) {
        Tally s, r;
        switch (ki) { case 0: run<2>(s, r); break; case 1: run<4>(s, r); break; case 2: run<6>(s, r); break; default: run<8>(s, r); }
        printf("%s\"k%d\": {\"single\": {\"n\": %ld, \"mismatch\": %ld, \"out_of_range\": %ld}, \"random\": {\"n\": %ld, \"mismatch\": %ld, \"out_of_range\": %ld}}",
               ki ? ", " : "", kOfIndex[ki], s.n, s.mismatch, s.out_of_range, r.n, r.mismatch, r.out_of_range);
        ok = ok && s.mismatch == 0 && r.mismatch == 0 && s.out_of_range == 0 && r.out_of_range == 0;
    }
    printf("}\n");
    return ok ? 0 : 1;
}
