// t3_rs_core.h — GF(27) Reed–Solomon RS(26,k) block decoder, shared by the host (superframe header,
// 2-3 blocks per frame) and the device (K4: one lane per flagged block).  Replaces
// RSCodec::decode_block (OLD:546-662).  Written over fixed-size coefficient arrays whose *lengths* follow
// the reference's std::vector sizes step for step, because the reference's results on garbage input
// (miscorrections, early `false`) depend on them and COMPAT mode must reproduce those bit for bit.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define T3_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define T3_HD inline
#endif

namespace t3 {

// Tables the decoder needs, laid out so one pointer serves host memory, __constant__ or LDS.
struct RsTables {
    uint8_t mul[729];   // a*27+b -> a.b              (GF27Context::mul OLD:473-476)
    uint8_t add[729];   // a*27+b -> a+b (trit-wise)  (gf27_add OLD:383-388)
    uint8_t neg[27];    // -a
    uint8_t inv[27];    // a^-1, inv[0]=0            (OLD:459-465)
    uint8_t exp[26];    // alpha^i                    (OLD:450-456)
    uint8_t pad_[3];
};

struct RsView {
    const uint8_t* mul; const uint8_t* add; const uint8_t* neg; const uint8_t* inv; const uint8_t* exp;
    T3_HD uint8_t M(uint8_t a, uint8_t b) const { return mul[a * 27 + b]; }
    T3_HD uint8_t A(uint8_t a, uint8_t b) const { return add[a * 27 + b]; }
    T3_HD uint8_t S(uint8_t a, uint8_t b) const { return add[a * 27 + neg[b]]; }
    T3_HD uint8_t P(int e) const { e %= 26; if (e < 0) e += 26; return exp[e]; }   // pow_alpha OLD:479-482
};

// Syndromes S_j = sum_i c_i alpha^{(j+1) i}, j = 0..R-1 (OLD:549-561). Returns true when all are zero.
template <int R>
T3_HD bool rs_syndromes(const RsView& g, const uint8_t* c, uint8_t* S) {
    bool zero = true;
#pragma unroll
    for (int j = 0; j < R; ++j) {
        uint8_t acc = 0;
#pragma unroll
        for (int i = 0; i < 26; ++i) acc = g.A(acc, g.M(c[i], g.exp[((j + 1) * i) % 26]));   // exponent is a compile-time constant
        S[j] = acc;
        zero = zero && acc == 0;
    }
    return zero;
}

// Everything after the syndromes: Berlekamp–Massey (OLD:567-605), Omega (OLD:606-610), Chien (OLD:611-624),
// formal derivative in characteristic 3 (OLD:625-641), Forney (OLD:642-659).
// fixed=false: reference behaviour, magnitude ADDED (OLD:658).  fixed=true: magnitude subtracted and the
// block is rejected unless L == deg(sigma) == #roots (bounded distance: a sigma shorter than the register that
// generates the syndromes locates nothing).  Corrects c in place; returns decode_block's bool.
template <int R>
T3_HD bool rs_correct(const RsView& g, uint8_t* c, const uint8_t* S, bool fixed) {
    constexpr int T = R / 2, NP = R + 2;          // polynomial lengths never exceed R+1
    uint8_t sg[NP], B[NP], tmp[NP];
    for (int i = 0; i < NP; ++i) { sg[i] = 0; B[i] = 0; }
    sg[0] = 1; B[0] = 1;
    int ns = 1, nB = 1, L = 0, m = 1;
    for (int n = 0; n < R; ++n) {
        uint8_t d = S[n];
        for (int i = 1; i <= L; ++i) if (i < ns) d = g.A(d, g.M(sg[i], S[n - i]));
        if (d != 0) {
            const int nsh = m + nB, nd = ns > nsh ? ns : nsh, nT = ns;
            for (int i = 0; i < NP; ++i) tmp[i] = sg[i];
            for (int i = 0; i < NP; ++i) {
                if (i >= nd) break;
                const uint8_t a = i < ns ? sg[i] : 0;
                const uint8_t b = (i >= m && i < nsh) ? g.M(d, B[i - m]) : 0;
                sg[i] = g.S(a, b);
            }
            ns = nd;
            if (2 * L <= n) {
                const uint8_t iv = g.inv[d];
                for (int i = 0; i < NP; ++i) B[i] = i < nT ? g.M(tmp[i], iv) : 0;
                nB = nT; L = n + 1 - L; m = 1;
            } else m += 1;
        } else m += 1;
    }
    uint8_t Om[R];                                  // (S(x) sigma(x)) mod x^R
    for (int q = 0; q < R; ++q) {
        uint8_t acc = 0;
        for (int j = 0; j < ns; ++j) if (j <= q) acc = g.A(acc, g.M(S[q - j], sg[j]));
        Om[q] = acc;
    }
    // Horner over the trailing zero coefficients of the reference's vector contributes nothing: start at the true degree
    int deg = ns - 1; while (deg > 0 && sg[deg] == 0) --deg;
    int pos[T + 1], np = 0;
    for (int i = 0; i < 26; ++i) {
        const uint8_t x = g.exp[i == 0 ? 0 : 26 - i];            // alpha^{-i}
        uint8_t acc = sg[deg];
        for (int q = deg - 1; q >= 0; --q) acc = g.A(g.M(acc, x), sg[q]);
        if (acc == 0) { if (np < T + 1) pos[np] = i; ++np; }
    }
    if (np > T) return false;
    if (fixed && (np != deg || L != deg)) return false;
    uint8_t dp[NP]; const int ndp = ns > 1 ? ns - 1 : 1;
    for (int i = 0; i < NP; ++i) dp[i] = 0;
    for (int i = 1; i < ns; ++i) { const int im = i % 3; dp[i - 1] = im == 0 ? 0 : (im == 1 ? sg[i] : g.A(sg[i], sg[i])); }
    int ddeg = ndp - 1; while (ddeg > 0 && dp[ddeg] == 0) --ddeg;
    for (int e = 0; e < np; ++e) {
        const uint8_t xi = g.exp[pos[e] == 0 ? 0 : 26 - pos[e]];
        uint8_t num = 0, den = dp[ddeg];
        for (int q = R - 1; q >= 0; --q) num = g.A(g.M(num, xi), Om[q]);
        for (int q = ddeg - 1; q >= 0; --q) den = g.A(g.M(den, xi), dp[q]);
        if (den == 0) return false;
        const uint8_t mag = g.M(g.neg[num], g.inv[den]);
        c[pos[e]] = fixed ? g.S(c[pos[e]], mag) : g.A(c[pos[e]], mag);
    }
    return true;
}

template <int R>
T3_HD bool rs_decode_block(const RsView& g, uint8_t* c, bool fixed) {
    uint8_t S[R];
    if (rs_syndromes<R>(g, c, S)) return true;
    return rs_correct<R>(g, c, S, fixed);
}

// ---- errors and erasures (FIXED arithmetic; include/t3hip.h, "repair with erasures") ---------------------------------------------
// mask: bit i set = position i is an erasure (its received byte was above 26); s = popcount(mask).  S: the R syndromes of the row with
// ANY value standing at the erased positions (the callers take the byte mod 27).  The block is accepted iff a codeword c exists with
// 2 e + s <= R, e = positions outside the mask where c differs from the row; then pos[0..n) / mag[0..n) are the erased positions (first,
// ascending; a magnitude may be 0) and the error positions, and c[pos] = row[pos] - mag.  n <= R.
//   Gamma(x) = prod_{l in mask} (1 - alpha^l x);  Xi = Gamma S mod x^R, whose coefficients s .. R-1 obey the ERROR locator's recurrence;
//   Berlekamp-Massey over those R - s;  roots of sigma over the positions outside the mask;  Psi = sigma Gamma, Omega = S Psi cut at
//   deg Psi (the register generates every modified syndrome, so the higher coefficients vanish);  magnitude = -Omega / Psi' at
//   alpha^-pos, the derivative in characteristic 3.
// Accepted in the FIXED style: register length = deg sigma = #roots outside the mask <= (R - s) / 2 (sigma has no more roots than its
// degree, so none sits on an erased position and every root of Psi is simple).  mask = 0 is rs_correct's FIXED rule.
// G: a field in RsView's shape -- M, A, S and neg[], inv[], exp[] (RsView itself; the fused kernels' LDS tables in t3_repair_era.hip).
template <int R, class G>
T3_HD bool rs_errata(const G& g, const uint8_t* S, const uint32_t mask, uint8_t* pos, uint8_t* mag, int& n) {
    constexpr int NP = R + 2;
    n = 0;
    int s = 0;
    for (int i = 0; i < 26; ++i) s += (int)((mask >> i) & 1u);
    if (s > R) return false;
    uint8_t Ga[NP];                                  // Gamma, degree s
    for (int i = 0; i < NP; ++i) Ga[i] = 0;
    Ga[0] = 1;
    {
        int dg = 0;
        for (int l = 0; l < 26; ++l) {
            if (!((mask >> l) & 1u)) continue;
            const uint8_t a = g.exp[l];
            for (int q = dg + 1; q >= 1; --q) Ga[q] = g.S(Ga[q], g.M(Ga[q - 1], a));
            ++dg;
        }
    }
    const int N = R - s;                             // modified syndromes the error locator must generate
    uint8_t Tm[R];
    for (int i = 0; i < R; ++i) Tm[i] = 0;
    for (int i = 0; i < N; ++i) {
        uint8_t acc = 0;
        for (int q = 0; q <= s; ++q) acc = g.A(acc, g.M(Ga[q], S[s + i - q]));
        Tm[i] = acc;
    }
    uint8_t sg[NP], B[NP], tmp[NP];
    for (int i = 0; i < NP; ++i) { sg[i] = 0; B[i] = 0; }
    sg[0] = 1; B[0] = 1;
    int L = 0, m = 1; uint8_t b = 1;
    for (int k = 0; k < N; ++k) {
        uint8_t d = Tm[k];
        for (int i = 1; i <= L; ++i) d = g.A(d, g.M(sg[i], Tm[k - i]));
        if (d == 0) { ++m; continue; }
        const uint8_t coef = g.M(d, g.inv[b]);
        const bool grow = 2 * L <= k;
        if (grow) for (int i = 0; i < NP; ++i) tmp[i] = sg[i];
        for (int i = m; i < NP; ++i) sg[i] = g.S(sg[i], g.M(coef, B[i - m]));
        if (grow) { for (int i = 0; i < NP; ++i) B[i] = tmp[i]; L = k + 1 - L; b = d; m = 1; } else ++m;
    }
    int deg = 0;
    for (int i = 1; i < NP; ++i) if (sg[i] != 0) deg = i;
    if (2 * L > N || deg != L) return false;
    // the erased positions first, then the roots of sigma outside the mask
    for (int i = 0; i < 26; ++i) if ((mask >> i) & 1u) pos[n++] = (uint8_t)i;
    int nr = 0;
    for (int i = 0; i < 26 && deg > 0; ++i) {
        if ((mask >> i) & 1u) continue;
        const uint8_t x = g.exp[i == 0 ? 0 : 26 - i];                    // alpha^-i
        uint8_t acc = sg[deg];
        for (int q = deg - 1; q >= 0; --q) acc = g.A(g.M(acc, x), sg[q]);
        if (acc == 0) { if (nr < deg) pos[n + nr] = (uint8_t)i; ++nr; }
    }
    if (nr != deg) { n = 0; return false; }
    n += nr;                                         // = deg Psi <= R
    uint8_t Ps[NP];                                  // Psi = sigma Gamma
    for (int i = 0; i < NP; ++i) {
        uint8_t acc = 0;
        for (int q = 0; q <= deg; ++q) if (q <= i && i - q <= s) acc = g.A(acc, g.M(sg[q], Ga[i - q]));
        Ps[i] = acc;
    }
    uint8_t Om[R];                                   // (S Psi) mod x^n
    for (int q = 0; q < R; ++q) {
        uint8_t acc = 0;
        if (q < n) for (int j = 0; j <= q; ++j) acc = g.A(acc, g.M(S[q - j], Ps[j]));
        Om[q] = acc;
    }
    uint8_t dp[NP];                                  // Psi', characteristic 3: i Psi_i with i mod 3
    for (int i = 0; i < NP; ++i) dp[i] = 0;
    for (int i = 1; i <= n; ++i) { const int im = i % 3; dp[i - 1] = im == 0 ? (uint8_t)0 : (im == 1 ? Ps[i] : g.A(Ps[i], Ps[i])); }
    for (int e = 0; e < n; ++e) {
        const uint8_t xi = g.exp[pos[e] == 0 ? 0 : 26 - pos[e]];
        uint8_t num = 0, den = 0;
        for (int q = n - 1; q >= 0; --q) { num = g.A(g.M(num, xi), Om[q]); den = g.A(g.M(den, xi), dp[q]); }
        if (den == 0) { n = 0; return false; }        // (a simple root: never)
        mag[e] = g.M(g.neg[num], g.inv[den]);
    }
    return true;
}

// One block, errors and erasures: c = the 26 symbols with the byte mod 27 at the erased positions.  Accepted: c becomes the codeword.
// Refused: c is left as it came.  mask = 0: rs_decode_block's FIXED decision, by that very function.
template <int R>
T3_HD bool rs_decode_block_erasures(const RsView& g, uint8_t* c, const uint32_t mask) {
    if (mask == 0) {
        uint8_t w[26];
        for (int i = 0; i < 26; ++i) w[i] = c[i];
        if (!rs_decode_block<R>(g, w, true)) return false;
        for (int i = 0; i < 26; ++i) c[i] = w[i];
        return true;
    }
    uint8_t S[R], pos[R], mag[R]; int n = 0;
    rs_syndromes<R>(g, c, S);
    if (!rs_errata<R>(g, S, mask, pos, mag, n)) return false;
    for (int e = 0; e < n; ++e) c[pos[e]] = g.S(c[pos[e]], mag[e]);
    return true;
}

}  // namespace t3
