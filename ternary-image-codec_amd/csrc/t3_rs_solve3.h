// t3_rs_solve3.h — RS(26,20) over GF(27): the error locator of a block with two or three errors in closed form, then roots, Omega and
// Forney as fx2_correct does them (t3_decode_fx2.h).  One text for the device (t3_decode_fx3.h: the field is the 27^3-byte multiply-add
// table in LDS) and for the host (tests/cpp/fx3_closed_form.cpp: the field's own tables), so what the CPU test proves is the kernel's code.
//
// Six syndromes S0..S5, Hankel matrix H3 = [[S0,S1,S2],[S1,S2,S3],[S2,S3,S4]] with the (symmetric) adjugate A.
//   D3 = det H3 != 0   no register shorter than 3 generates the syndromes, and exactly one of length 3 does:
//                      (s3, s2, s1) = -A (S3, S4, S5)^T / D3.  It is the register Berlekamp-Massey returns (2 L <= 6: unique).
//   D3 = 0, D2 = A22 = S0 S2 - S1^2 != 0
//                      the length-2 register through S0..S3 is s1 = A12 / D2, s2 = A02 / D2 (Cramer).  It generates S4 and S5 as well iff
//                      D2 S4 + A12 S3 + A02 S2 = 0 -- which is D3 expanded along its last row, known to be 0 -- and
//                      D2 S5 + A12 S4 + A02 S3 = 0 (N1 below).  Then it is unique again, and Berlekamp-Massey's.
//   anything else      not decided here: L = 0, the caller runs Berlekamp-Massey.
// A locator of lower degree than its length (s3 = 0, or s2 = 0 with L = 2) has fewer roots than L and ends in the same place, as do a
// root count != L and a zero Forney denominator: only the fallback ever refuses a block.
//
// F, the field: mad(a, x, y) = a + x y, neg(x), inv(x), ninv(x) = -1 / x (x != 0), ex(i) = alpha^i (i < 26) and
// roots(i) = the 26-bit mask of the positions p with 1 + s1 x + s2 x^2 + s3 x^3 = 0 at x = alpha^-p, i = s1 + 27 s2 + 729 s3.
#pragma once
#include <stdint.h>

#include "t3_rs_core.h"

namespace t3 {

struct Solve3 { uint32_t np; uint32_t pos[3], mag[3]; };     // np = 0: fallback; else np = L in {2, 3} corrections, c[pos] -= mag

template <int R, class F>
T3_HD Solve3 fx2_solve(const F& f, const uint32_t* S) {
    static_assert(R == 6, "closed form for t = 3 only");
    // cofactors: products side by side, then one more level each
    const uint32_t n1 = f.neg(S[1]), n2 = f.neg(S[2]), n3 = f.neg(S[3]);
    const uint32_t A00 = f.mad(f.mad(0u, S[2], S[4]), n3, S[3]);       // S2 S4 - S3^2
    const uint32_t A01 = f.mad(f.mad(0u, S[2], S[3]), n1, S[4]);       // S2 S3 - S1 S4
    const uint32_t A02 = f.mad(f.mad(0u, S[1], S[3]), n2, S[2]);       // S1 S3 - S2^2
    const uint32_t A11 = f.mad(f.mad(0u, S[0], S[4]), n2, S[2]);       // S0 S4 - S2^2
    const uint32_t A12 = f.mad(f.mad(0u, S[1], S[2]), n3, S[0]);       // S1 S2 - S0 S3
    const uint32_t A22 = f.mad(f.mad(0u, S[0], S[2]), n1, S[1]);       // S0 S2 - S1^2
    // four independent three-term chains
    const uint32_t D3 = f.mad(f.mad(f.mad(0u, S[0], A00), S[1], A01), S[2], A02);
    const uint32_t N3 = f.mad(f.mad(f.mad(0u, S[3], A00), S[4], A01), S[5], A02);
    const uint32_t N2 = f.mad(f.mad(f.mad(0u, S[3], A01), S[4], A11), S[5], A12);
    const uint32_t N1 = f.mad(f.mad(f.mad(0u, S[3], A02), S[4], A12), S[5], A22);
    const bool three = D3 != 0u, two = D3 == 0u && A22 != 0u && N1 == 0u;
    const uint32_t L = three ? 3u : two ? 2u : 0u;
    const uint32_t iv = three ? f.ninv(D3) : f.inv(two ? A22 : 1u);
    const uint32_t s1 = f.mad(0u, iv, three ? N1 : A12), s2 = f.mad(0u, iv, three ? N2 : A02), s3 = f.mad(0u, iv, three ? N3 : 0u);
    const uint32_t roots = f.roots(L != 0u ? s1 + 27u * (s2 + 27u * s3) : 0u);
    const uint32_t np = (uint32_t)__builtin_popcount(roots);
    // Omega = S sigma mod x^6 cut at x^3 (degree < L here), sigma' = s1 + 2 s2 x in characteristic 3
    const uint32_t Om1 = f.mad(S[1], S[0], s1), Om2 = f.mad(f.mad(S[2], S[1], s1), S[0], s2);
    const uint32_t s22 = f.mad(s2, 1u, s2);
    Solve3 r;
    bool bad = L == 0u || np != L;
    uint32_t rm = roots, xi[3];
#pragma unroll
    for (int e = 0; e < 3; ++e) {                                        // a slot without a root runs on position 0 and is discarded
        const bool have = (uint32_t)e < np && rm != 0u;
        const uint32_t p = have ? (uint32_t)__builtin_ctz(rm) : 0u; rm &= rm - 1u;
        r.pos[e] = p; xi[e] = f.ex(p == 0u ? 0u : 26u - p);
    }
#pragma unroll
    for (int e = 0; e < 3; ++e) {
        const uint32_t den = f.mad(s1, xi[e], s22);
        const uint32_t num = f.mad(S[0], xi[e], f.mad(Om1, xi[e], Om2));
        bad = bad || ((uint32_t)e < np && den == 0u);
        r.mag[e] = f.mad(0u, f.neg(num), f.inv(den));
    }
    r.np = bad ? 0u : np;
    return r;
}

}  // namespace t3
