// t3_enc_convert.h — phase 1 of the fused encoder (t3_encode.h): input bytes -> stream-ordered symbols in LDS.  Device-only,
// header-inline.  The small converters also serve the RAW packer (t3_kernels.hip).
//   small converters     red_y, red_c, px3_to_sym13, w3_to_sym26, px3x2_to_sym13x8, rgb_px_to_comps
//   2-D geometry         il_perm, IlCursor, enc_row, IlRuns / il_runs
//   input -> LDS         stage_input (LDS-DMA), convert_groups (the row-by-row flow of raw words in 2-D)
//   packed converters    P1Run / p1_run, convert_pixels_packed; W1Run / w1_run, convert_words_half, convert_words_packed
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "t3_device.h"
#include "t3_devutil.h"

namespace t3 {

typedef uint32_t u32x2a4 __attribute__((ext_vector_type(2), aligned(4)));

// Components as the reference's i2tr sees them: v % 3^w of the uint32 cast (no clamping, OLD:675-682,697-702).
// 16-bit operands: floor(x/d) = floor((x + 0.5) * fl(1/d)) exactly for x < 65536 (the +0.5 keeps the product
// >= 0.5/d away from every integer, far more than the float rounding error).
__device__ __forceinline__ uint32_t red_y(uint32_t y16) {
    const uint32_t q = (uint32_t)(((float)y16 + 0.5f) * (1.0f / 243.0f));
    return y16 - __umul24(q, 243u);
}
__device__ __forceinline__ uint32_t red_c(uint32_t c16) {
    const int32_t v = (int32_t)(int16_t)c16 + 40;
    // negative v: (2^32 + v) % 81 = (v + 49 + 81*405) % 81, and v + 32854 > 0 for every int16
    const uint32_t x = v < 0 ? (uint32_t)(v + 32854) : (uint32_t)v;
    const uint32_t q = (uint32_t)(((float)x + 0.5f) * (1.0f / 81.0f));
    return x - __umul24(q, 81u);
}

// 3 pixels = 39 trits = 13 symbols (trit t of the stream = trit t%13 of pixel t/13; Y:5, Cb+40:4, Cr+40:4).
// Every symbol is a div/mod-by-power-of-3 splice of at most two components — no per-trit work.
__device__ __forceinline__ void px3_to_sym13(const uint32_t* c /*9 reduced comps*/, uint32_t* s /*13*/) {
    const uint32_t Y0 = c[0], B0 = c[1], R0 = c[2], Y1 = c[3], B1 = c[4], R1 = c[5], Y2 = c[6], B2 = c[7], R2 = c[8];
    uint32_t q;
    q = div27(Y0); s[0] = Y0 - 27u * q;            s[1] = q + 9u * mod3(B0);
    s[2] = div3(B0);
    q = div27(R0); s[3] = R0 - 27u * q;            s[4] = q + 3u * mod9(Y1);
    s[5] = div9(Y1);
    q = div27(B1); s[6] = B1 - 27u * q;            s[7] = q + 3u * mod9(R1);
    s[8] = div9(R1) + 9u * mod3(Y2);
    s[9] = mod27(div3(Y2));
    s[10] = div81(Y2) + 3u * mod9(B2);
    s[11] = div9(B2) + 9u * mod3(R2);
    s[12] = div3(R2);
}

// 3 raw words (27 canonical symbols, trit 26 of each dropped, OLD:1065-1076) = 78 trits = 26 symbols.
__device__ __forceinline__ void w3_to_sym26(const uint32_t* c /*27 symbols < 27*/, uint32_t* s /*26*/) {
#pragma unroll
    for (int i = 0; i < 8; ++i) s[i] = c[i];
    s[8] = mod9(c[8]) + 9u * mod3(c[9]);
#pragma unroll
    for (int i = 0; i < 8; ++i) s[9 + i] = div3(c[9 + i]) + 9u * mod3(c[10 + i]);
    s[17] = mod3(div3(c[17])) + 3u * mod9(c[18]);
#pragma unroll
    for (int i = 0; i < 8; ++i) s[18 + i] = div9(c[18 + i]) + 3u * mod9(c[19 + i]);
}

// 2-D boustrophedon position map (an involution inside each row segment; OLD:750-780)
__device__ __forceinline__ uint32_t il_perm(uint32_t u, const EncArgs& a) {
    const uint32_t chunk = div_ge2(u, a.div_A), base = chunk * a.il_A, rem = u - base;
    const uint32_t take = min(a.il_A, a.n_sym - base);
    const uint32_t r = div_ge2(rem, a.div_w), c = rem - r * a.il_w;
    const uint32_t rowlen = min(a.il_w, take - r * a.il_w);
    return base + r * a.il_w + ((r & 1u) ? rowlen - 1u - c : c);
}
// The same map for a run of consecutive positions: one pair of divisions at the start, then a few compares per step
struct IlCursor {
    uint32_t base, take, rw, c, rowlen, odd;                 // chunk start, chunk size, row start in the chunk, column, row length, row parity
    __device__ __forceinline__ void init(uint32_t u, const EncArgs& a) {
        const uint32_t chunk = div_ge2(u, a.div_A); base = chunk * a.il_A;
        const uint32_t rem = u - base; take = min(a.il_A, a.n_sym - base);
        const uint32_t r = div_ge2(rem, a.div_w); rw = r * a.il_w; c = rem - rw; odd = r & 1u;
        rowlen = min(a.il_w, take - rw);
    }
    __device__ __forceinline__ uint32_t get() const { return base + rw + (odd ? rowlen - 1u - c : c); }
    __device__ __forceinline__ void next(const EncArgs& a, const uint32_t step = 1u) {     // step 4: rows that are multiples of 4
        c += step;
        if (c >= rowlen) {
            c = 0; rw += a.il_w; odd ^= 1u;
            if (rw >= take) { base += a.il_A; take = min(a.il_A, a.n_sym - base); rw = 0; odd = 0; }
            rowlen = min(a.il_w, take - rw);
        }
    }
};
// Row segment of position u (t3_devutil.h); branch-free division: rows of one symbol never get here
__device__ __forceinline__ IlRow enc_row(uint32_t u, const EncArgs& a) { return il_row_of<div_ge2>(u, a.n_sym, a.il_w, a.il_A, a.div_A, a.div_w); }
// The pre-interleave symbols that land in the post-interleave tile [S0, S0 + TS): the map is an involution inside every row
// segment, so whole rows of the tile come from themselves and only the tile's partial first / last row comes from the mirrored
// piece of that row -- at most three runs of consecutive pre-interleave positions (ascending, adjacent ones merged), TS symbols
// in all, whatever the row width.  Positions past the end of the stream map to themselves.
struct IlRuns { uint32_t lo[3], hi[3], plo[3], n; };      // plo: post-interleave position of the run's lowest-placed symbol (its symbols occupy [plo, plo + hi - lo) of the tile)
__device__ __forceinline__ IlRuns il_runs(uint32_t S0, uint32_t TS, const EncArgs& a) {
    IlRuns R; R.n = 0; R.lo[0] = R.lo[1] = R.lo[2] = 0; R.hi[0] = R.hi[1] = R.hi[2] = 0; R.plo[0] = R.plo[1] = R.plo[2] = 0;
    auto push = [&](uint32_t lo, uint32_t hi, uint32_t plo) {                  // (no dynamic indexing: the runs stay in registers)
        if (lo >= hi) return;
        // adjacent runs are merged when their places are adjacent too (identity-placed neighbours; a mirrored piece never is)
        if (R.n == 0u) { R.lo[0] = lo; R.hi[0] = hi; R.plo[0] = plo; R.n = 1u; }
        else if (R.n == 1u) { if (R.hi[0] == lo && R.plo[0] + (R.hi[0] - R.lo[0]) == plo) R.hi[0] = hi; else { R.lo[1] = lo; R.hi[1] = hi; R.plo[1] = plo; R.n = 2u; } }
        else if (R.n == 2u) { if (R.hi[1] == lo && R.plo[1] + (R.hi[1] - R.lo[1]) == plo) R.hi[1] = hi; else { R.lo[2] = lo; R.hi[2] = hi; R.plo[2] = plo; R.n = 3u; } }
        else if (R.hi[2] == lo) R.hi[2] = hi;
    };
    const uint32_t E = min(S0 + TS, a.n_sym);
    if (S0 < E) {
        // (il_row_of's arithmetic, left written out here with reference outputs: through enc_row the run ends below came out re-associated,
        // two scalar instructions fewer inside the tile loop of every run-placed 2-D kernel, and that was not timed)
        auto il_row = [&](uint32_t u, uint32_t& rl, uint32_t& rn, uint32_t& odd) {
            const uint32_t chunk = div_ge2(u, a.div_A), base = chunk * a.il_A, rem = u - base;
            const uint32_t take = min(a.il_A, a.n_sym - base);
            const uint32_t r = div_ge2(rem, a.div_w);
            rl = base + r * a.il_w; rn = min(a.il_w, take - r * a.il_w); odd = r & 1u;
        };
        uint32_t rl0, rn0, od0, rl1, rn1, od1;
        il_row(S0, rl0, rn0, od0); il_row(E - 1u, rl1, rn1, od1);
        if (rl0 == rl1) push(od0 ? rl0 + rn0 - (E - rl0) : S0, od0 ? rl0 + rn0 - (S0 - rl0) : E, S0);
        else {
            const uint32_t he = rl0 + rn0;
            push(od0 ? rl0 : S0, od0 ? he - (S0 - rl0) : he, S0);
            push(he, rl1, he);
            push(od1 ? rl1 + rn1 - (E - rl1) : rl1, od1 ? rl1 + rn1 : E, rl1);
        }
    }
    push(max(S0, a.n_sym), S0 + TS, max(S0, a.n_sym));
    return R;
}

// Stage the input bytes of lane groups [g_lo, g_hi) into the stage buffer at LDS offset `stage`: image byte x = input
// byte b0 + x with b0 = 16-aligned start of group g_lo.  Whole 1-KiB pieces inside the real data go by LDS-DMA
// (global_load_lds_dwordx4: no VGPR round trip, completes behind vmcnt, so the next tile's input streams in under
// this tile's compute); pieces that touch the end of the data are synthesised (pad pixel OLD:730, then zero trits).
constexpr int kDmaAux = 3;   // cache policy of the input LDS-DMA: sc0 | nt (the input is read once; measured 2-3 % over the default policy, profiles/r02/notes.md)
template <int FE>
__device__ __forceinline__ void stage_input(const EncArgs& a, uint32_t stage, uint32_t g_lo, uint32_t g_hi, uint32_t lane, uint32_t wave, uint32_t nwv, const uint64_t base = 0) {   // base: the frame's byte offset from a.in (batch launches)
    constexpr uint32_t GB = FE == FE_PIXELS ? kGroupBytes : FE == FE_RGB ? kGroupBytesRgb : kGroupBytesW, UB = FE == FE_PIXELS ? 6u : FE == FE_RGB ? 3u : 9u;
    const uint64_t b0 = ((uint64_t)g_lo * GB) & ~15ull, b1 = (uint64_t)g_hi * GB, real = a.n_units * UB;
    const uint32_t n_chunks = (uint32_t)((b1 - b0 + 15u) >> 4);
    for (uint32_t c0 = __builtin_amdgcn_readfirstlane(wave) * 64u; c0 < n_chunks; c0 += nwv * 64u) {
        const uint64_t o = b0 + 16ull * (c0 + lane);
        if (b0 + 16ull * (c0 + 64u) <= real) {
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) uint32_t*)(a.in + base + o),
                                             (__attribute__((address_space(3))) uint32_t*)(lds + stage + 16u * c0), 16, 0, kDmaAux);
        } else if (c0 + lane < n_chunks) {
            uint32_t w[4] = {0, 0, 0, 0};
            if (o + 16u <= real) { const uint4 v = *(const uint4*)(a.in + base + o); w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w; }
            else if constexpr (FE == FE_PIXELS) {
#pragma unroll
                for (int h = 0; h < 8; ++h) {
                    const uint64_t n = (o >> 1) + h, px = n / 3u; const uint32_t comp = (uint32_t)(n - 3u * px);
                    uint32_t val;
                    if (px < a.n_units) val = *(const uint16_t*)(a.in + base + 2u * n);
                    else if (px < a.n_units_pad) val = 0u;
                    else val = comp == 0 ? 0u : 0xFFD8u;                          // -40 -> Cb+40 = 0
                    w[h >> 1] |= val << (16 * (h & 1));
                }
            } else {                                                              // raw words, RGB: bytes past the end read as zero (RGB black = the pad pixel)
#pragma unroll
                for (int h = 0; h < 16; ++h) { const uint64_t n = o + h; if (n < real) w[h >> 2] |= (uint32_t)(a.in + base)[n] << (8 * (h & 3)); }
            }
            *(uint4*)(lds + stage + 16u * (c0 + lane)) = make_uint4(w[0], w[1], w[2], w[3]);
        }
    }
}

// Phase 1: lane groups [g_lo, g_hi) of the stage buffer -> stream-ordered symbols [S0, S0+TS) in LDS.
template <int FE, bool IL, int SH>     // SH: symbols are stored pre-scaled by 2^SH (the byte offset of their table entry)
__device__ __forceinline__ void convert_groups(const EncArgs& a, uint32_t stage, uint32_t g_base, uint32_t g_lo, uint32_t g_hi,
                                               uint32_t S0, uint32_t TS, uint32_t tid, uint32_t nthr) {
    constexpr uint32_t GS = FE == FE_PIXELS ? kGroupSyms : kGroupSymsW, GB = FE == FE_PIXELS ? kGroupBytes : kGroupBytesW;
    constexpr uint32_t QS = GS / 2;                                        // 3 px -> 13 symbols, 3 words -> 26 symbols
    constexpr uint32_t EM = FE == FE_PIXELS ? 2u : 4u;                     // bytes per LDS store on the fast path (26 g is 2-aligned)
    const uint64_t b0 = ((uint64_t)g_base * GB) & ~15ull;
    for (uint32_t g0 = g_lo; g0 < g_hi; g0 += nthr) {                      // wave-uniform trip count (ballots inside)
        if (g0 + (tid & ~63u) >= g_hi) break;                                // a wave without a live lane has nothing to convert (the ballots are per wave)
        const uint32_t g = g0 + tid; const bool live = g < g_hi;
        const uint32_t src = stage + (uint32_t)((uint64_t)(live ? g : g_lo) * GB - b0);
        const uint32_t u0 = g * GS;
        const bool whole = !IL && u0 >= S0 && u0 + GS <= S0 + TS;         // whole group lands in the tile: wide stores
        const uint32_t dst = a.sym_off + (u0 - S0);
        uint32_t acc = 0;
#pragma unroll
        for (uint32_t q = 0; q < 2; ++q) {
            uint32_t sq[QS];
            if constexpr (FE == FE_PIXELS) {
                uint32_t h[9], c[9]; bool bad = false;
#pragma unroll
                for (uint32_t i = 0; i < 9; ++i) {
                    h[i] = *(const uint16_t*)(lds + src + 18u * q + 2u * i);
                    c[i] = (i % 3 == 0) ? h[i] : ((h[i] + 40u) & 0xFFFFu);
                    bad |= c[i] >= ((i % 3 == 0) ? 243u : 81u);
                }
                if (__builtin_amdgcn_ballot_w64(bad) != 0) {                // out-of-range quantised values: exact general reduction
#pragma unroll
                    for (uint32_t i = 0; i < 9; ++i) c[i] = (i % 3 == 0) ? red_y(h[i]) : red_c(h[i]);
                }
                px3_to_sym13(c, sq);
            } else {
                uint32_t c[27]; bool bad = false;
                // the half group's 27 bytes as 14 halfwords (groups are 2-byte aligned; q = 1 starts on an odd byte)
                uint32_t hb[28];
#pragma unroll
                for (uint32_t i = 0; i < 14; ++i) { const uint32_t h = *(const uint16_t*)(lds + src + 26u * q + 2u * i); hb[2 * i] = h & 0xFFu; hb[2 * i + 1] = h >> 8; }
#pragma unroll
                for (uint32_t i = 0; i < 27; ++i) { c[i] = hb[q + i]; bad |= c[i] >= 27u; }
                if (__builtin_amdgcn_ballot_w64(bad) != 0) {
#pragma unroll
                    for (uint32_t i = 0; i < 27; ++i) c[i] = mod27(c[i]);
                }
                w3_to_sym26(c, sq);
            }
            if (live && whole) {
#pragma unroll
                for (uint32_t i = 0; i < QS; ++i) {
                    const uint32_t n = q * QS + i;
                    acc |= sq[i] << ((uint32_t)SH + 8u * (n % EM));            // stored pre-scaled (table entry offset)
                    if (n % EM == EM - 1u) {
                        if constexpr (EM == 2u) *(uint16_t*)(lds + dst + (n - 1u)) = (uint16_t)acc; else *(uint32_t*)(lds + dst + (n - 3u)) = acc;
                        acc = 0;
                    }
                }
            } else if (!IL && live) {
                // group straddles a tile edge (tile edges are multiples of 4, group starts are even): same wide stores, predicated
#pragma unroll
                for (uint32_t i = 0; i < QS; ++i) {
                    const uint32_t n = q * QS + i;
                    acc |= sq[i] << ((uint32_t)SH + 8u * (n % EM));
                    if (n % EM == EM - 1u) {
                        const uint32_t u = u0 + n - (EM - 1u);
                        if (u >= S0 && u + EM <= S0 + TS) {
                            if constexpr (EM == 2u) *(uint16_t*)(lds + dst + (n - 1u)) = (uint16_t)acc; else *(uint32_t*)(lds + dst + (n - 3u)) = acc;
                        }
                        acc = 0;
                    }
                }
            } else if (live) {
                IlCursor cur;
                if constexpr (IL) { if (u0 + q * QS < a.n_sym) cur.init(u0 + q * QS, a); }
#pragma unroll
                for (uint32_t i = 0; i < QS; ++i) {
                    uint32_t u = u0 + q * QS + i;
                    if constexpr (IL) { if (u >= a.n_sym) continue; u = cur.get(); cur.next(a); }
                    if (u >= S0 && u < S0 + TS) lds[a.sym_off + (u - S0)] = (uint8_t)(sq[i] << SH);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------
// Phase 1 for pixels, packed: one lane converts TWO pixel triples at once with 16-bit packed VALU ops (v_pk_*): component
// i of triple A sits in the low half of a register, of triple B = A+2 in the high half (ds_read_u16 + ds_read_u16_d16_hi),
// every product stays below 2^16.  Both triples of a lane have the same parity, and a wave handles one parity only, so the
// byte pairing of the 13 output symbols (offset 13t is odd for odd t) is wave-uniform: 6 b16 stores + 1 b8 store per triple.
// ---------------------------------------------------------------------------------------------------------

// 9 reduced components (Y < 243, C < 81) of a triple pair -> 13 symbol pairs, each already multiplied by SC
template <int SC>
__device__ __forceinline__ void px3x2_to_sym13x8(const u16x2* c, u16x2* s) {
    const u16x2 Y0 = c[0], B0 = c[1], R0 = c[2], Y1 = c[3], B1 = c[4], R1 = c[5], Y2 = c[6], B2 = c[7], R2 = c[8];
    const uint16_t k8 = SC, k24 = 3 * SC, k72 = 9 * SC, k216 = 27 * SC;
    u16x2 q, t;
    q = pk_d27(Y0); s[0] = Y0 * k8 - q * k216;            t = pk_d3(B0);  s[1] = q * k8 + (B0 - t * (uint16_t)3) * k72;  s[2] = t * k8;
    q = pk_d27(R0); s[3] = R0 * k8 - q * k216;            t = pk_d9(Y1);  s[4] = q * k8 + (Y1 - t * (uint16_t)9) * k24;  s[5] = t * k8;
    q = pk_d27(B1); s[6] = B1 * k8 - q * k216;            t = pk_d9(R1);  s[7] = q * k8 + (R1 - t * (uint16_t)9) * k24;
    const u16x2 y3 = pk_d3(Y2), y9 = pk_d9(Y2), y81 = pk_d9(y9);                                  // Y2/3, Y2/9, Y2/81
    s[8] = t * k8 + (Y2 - y3 * (uint16_t)3) * k72;
    s[9] = y3 * k8 - y81 * k216;                                                                   // (Y2/3) % 27 = Y2/3 - 27 (Y2/81)
    t = pk_d9(B2);  s[10] = y81 * k8 + (B2 - t * (uint16_t)9) * k24;
    q = pk_d3(R2);  s[11] = t * k8 + (R2 - q * (uint16_t)3) * k72;  s[12] = q * k8;
}

// Convert the pixel triples that cover stream symbols [S0, S0+TS) from the stage buffer (image byte x = input byte b0 + x).
// A lane takes FOUR consecutive triples (12 pixels, 72 input bytes -> 52 symbols): its input is nine aligned 8-byte reads, its
// output thirteen aligned dwords.  Triples 0 and 2 share registers as low/high halves, so do 1 and 3 (same parity each).
// Triples are written whole: the symbol buffer has kSymFront bytes of slack in front and 64 behind, which take the symbols of
// the first/last triples that belong to the neighbouring tiles (and of the up to three triples past the tile's last one).
// Symbols [u_lo, u_hi) are produced (1-D: the tile itself; pipelined 2-D: the row segments it overlaps); symbol u lands at
// LDS byte sym_off + (u - u_lo).
// FE_RGB: the io_image.hpp bridge for one pixel (rgb_to_ycbcr :47-57, quantize_ycbcr :69-78): every float product and sum rounded on
// its own (no contraction), std::lround of a non-negative value = trunc(x + 0.5) exactly (x + 0.5 is exact or rounds inside
// the integer's unit interval), Y quantised in float (242 Y / 255 is never within 1/510 of a tie, the float error is 1e-5),
// chroma through the 256-byte table of its quantiser.  Returns the reduced components Y < 243, Cb + 40, Cr + 40 <= 80.
__device__ __forceinline__ void rgb_px_to_comps(const uint32_t r8, const uint32_t g8, const uint32_t b8, const uint32_t qt, uint32_t& Y, uint32_t& B, uint32_t& R) {
    const float r = (float)r8, g = (float)g8, b = (float)b8;
    const float y = __fadd_rn(__fadd_rn(__fmul_rn(0.299f, r), __fmul_rn(0.587f, g)), __fmul_rn(0.114f, b));
    const float cb = __fadd_rn(__fadd_rn(__fsub_rn(__fmul_rn(-0.168736f, r), __fmul_rn(0.331264f, g)), __fmul_rn(0.5f, b)), 128.0f);
    const float cr = __fadd_rn(__fsub_rn(__fsub_rn(__fmul_rn(0.5f, r), __fmul_rn(0.418688f, g)), __fmul_rn(0.081312f, b)), 128.0f);
    const float Yi = fminf(truncf(__fadd_rn(y, 0.5f)), 255.0f);
    Y = (uint32_t)__fmaf_rn(Yi, 242.0f / 255.0f, 0.5f);
    const uint32_t Cb = min((uint32_t)__fadd_rn(cb, 0.5f), 255u), Cr = min((uint32_t)__fadd_rn(cr, 0.5f), 255u);
    B = lds_u8(qt + Cb); R = lds_u8(qt + Cr);
}

// One run of consecutive pixel triples for phase 1: triples [t_base, t_end) in lane units of four (t_base a multiple of 4); triple t
// reads its input at LDS address src0 + t * (18 | 9) (pixels | RGB)
struct P1Run { uint32_t t_base, t_end, n_units, src0, lo, hi, dst0; };   // lo, hi, dst0: run-placed 2-D flow (symbol u of [lo, hi) goes to LDS address dst0 + u)
template <int FE>
__device__ __forceinline__ P1Run p1_run(uint32_t u_lo, uint32_t u_hi, uint32_t stage) {    // symbols [u_lo, u_hi), their input staged at `stage` (see stage_input)
    constexpr uint32_t GBf = FE == FE_PIXELS ? kGroupBytes : kGroupBytesRgb, TB = FE == FE_PIXELS ? 18u : 9u;
    P1Run r; r.t_base = (u_lo / 13u) & ~3u; r.t_end = (u_hi + 12u) / 13u; r.n_units = (r.t_end - r.t_base + 3u) / 4u;
    const uint64_t b0 = ((uint64_t)(r.t_base / 2u) * GBf) & ~15ull;                       // 16-aligned start of the first lane group (two triples each)
    r.src0 = stage - (uint32_t)b0;                                                       // (wraps; src0 + t * TB does not)
    r.lo = u_lo; r.hi = u_hi; r.dst0 = 0;
    (void)TB;
    return r;
}

// IL: the symbols go to their post-interleave places in the tile [S0, S0 + TS) (what falls outside belongs to another tile);
// else symbol u goes to sym_off + (u - S0).
// placed (IL only, wave-uniform): the run-placed flow -- a run's symbols go, in pre-interleave order, to the place the run occupies in the
// tile (P1Run::dst0; rows, chunks and tile edges are multiples of 4 there, so aligned dwords stay aligned dwords) and the caller
// reverses the odd rows' pieces in place afterwards.
template <int SC, int FE, bool IL>
__device__ __forceinline__ void convert_pixels_packed(const EncArgs& a, const P1Run r0, const P1Run r1, const P1Run r2, uint32_t S0, uint32_t TS,
                                                      uint32_t lane, uint32_t wave, uint32_t nwv, const bool placed = false) {
    constexpr uint32_t TB = FE == FE_PIXELS ? 18u : 9u;
    const uint32_t nw1 = min(a.p1_wpp, nwv);                                      // waves that convert (planner: just enough lanes)
    if (wave >= nw1) return;
    const uint32_t n0 = r0.n_units, n01 = IL ? n0 + r1.n_units : n0, n_all = IL ? n01 + r2.n_units : n0;      // (separate values, not an array: selects, no private memory)
    for (uint32_t e0 = wave * 64u; e0 < n_all; e0 += nw1 * 64u) {
        const uint32_t e = e0 + lane;
        const uint32_t ri = !IL ? 0u : e < n0 ? 0u : e < n01 ? 1u : 2u;            // (1-D: one run)
        const uint32_t t_base = ri == 0u ? r0.t_base : ri == 1u ? r1.t_base : r2.t_base;
        const uint32_t t_end = ri == 0u ? r0.t_end : ri == 1u ? r1.t_end : r2.t_end;
        const uint32_t src0 = ri == 0u ? r0.src0 : ri == 1u ? r1.src0 : r2.src0;
        const uint32_t t = t_base + 4u * (e - (ri == 0u ? 0u : ri == 1u ? n0 : n01));
        const bool live = t < t_end;
        u16x2 sA[13], sB[13];
        if constexpr (FE == FE_RGB) {
            // 12 pixels = 36 bytes = nine aligned dwords; pixel p = bytes 3p .. 3p + 2
            const uint32_t src = src0 + (live ? t : t_base) * TB;
            uint32_t D[9];
#pragma unroll
            for (uint32_t i = 0; i < 9; ++i) D[i] = lds_u32(src + 4u * i);
            // pixels past the padded end of the frame are zero TRITS (Cb + 40 = 0), which no RGB value encodes: only the frame's last lanes
            const uint64_t px0 = 3ull * t;
            const bool tail = __builtin_amdgcn_ballot_w64(live && px0 + 12u > a.n_units_pad) != 0;
            auto byte = [&](uint32_t k) -> uint32_t { return (D[k >> 2] >> (8u * (k & 3u))) & 0xFFu; };
#pragma unroll
            for (uint32_t pair = 0; pair < 2; ++pair) {                           // pair 0 = triples (0, 2), pair 1 = triples (1, 3): six pixels at a time (register budget)
                u16x2 c[9];
#pragma unroll
                for (uint32_t m = 0; m < 3; ++m) {
                    const uint32_t pa = 3u * pair + m, pb = pa + 6u;              // pixel of the pair's first / second triple
                    uint32_t Ya, Ba, Ra, Yb, Bb, Rb;
                    rgb_px_to_comps(byte(3u * pa), byte(3u * pa + 1u), byte(3u * pa + 2u), a.qt_off, Ya, Ba, Ra);
                    rgb_px_to_comps(byte(3u * pb), byte(3u * pb + 1u), byte(3u * pb + 2u), a.qt_off, Yb, Bb, Rb);
                    if (tail) {
                        if (px0 + pa >= a.n_units_pad) { Ya = 0; Ba = 0; Ra = 0; }
                        if (px0 + pb >= a.n_units_pad) { Yb = 0; Bb = 0; Rb = 0; }
                    }
                    c[3 * m] = u16x2{(uint16_t)Ya, (uint16_t)Yb}; c[3 * m + 1] = u16x2{(uint16_t)Ba, (uint16_t)Bb}; c[3 * m + 2] = u16x2{(uint16_t)Ra, (uint16_t)Rb};
                }
                px3x2_to_sym13x8<SC>(c, pair ? sB : sA);
            }
        } else {
        const uint32_t src = src0 + (live ? t : t_base) * TB;                             // 8-byte aligned
        uint32_t D[18];
#pragma unroll
        for (uint32_t i = 0; i < 9; ++i) { const u32x2 v = *T3_LDS(const u32x2, src + 8u * i); D[2 * i] = v.x; D[2 * i + 1] = v.y; }
        // halves whose triple lies past the tile's last one hold stale bytes: keep them out of the range check
        const uint32_t liveA = t + 2u < t_end ? 0xFFFFFFFFu : 0x0000FFFFu, liveB = (t + 1u < t_end ? 0x0000FFFFu : 0u) | (t + 3u < t_end ? 0xFFFF0000u : 0u);
#pragma unroll
        for (uint32_t pair = 0; pair < 2; ++pair) {                               // pair 0 = triples (0, 2), pair 1 = triples (1, 3)
            u16x2 h[9], c[9];
            u16x2 mxY = {0, 0}, mxC = {0, 0};                                    // range check on the maxima: one comparison per kind instead of one per component
#pragma unroll
            for (uint32_t i = 0; i < 9; ++i) {
                const uint32_t u = 9u * pair + i;                                 // 16-bit index of the low-half component; the high half sits 18 further
                const uint32_t w = __builtin_amdgcn_perm(D[9u + u / 2u], D[u / 2u], (u & 1u) ? 0x07060302u : 0x05040100u);
                h[i] = __builtin_bit_cast(u16x2, w);
                c[i] = (i % 3 == 0) ? h[i] : h[i] + (uint16_t)40;
                if (i % 3 == 0) mxY = __builtin_elementwise_max(mxY, c[i]); else mxC = __builtin_elementwise_max(mxC, c[i]);
            }
            const u16x2 over = __builtin_elementwise_sub_sat(mxY, (u16x2)((uint16_t)242)) | __builtin_elementwise_sub_sat(mxC, (u16x2)((uint16_t)80));
            if (__builtin_amdgcn_ballot_w64(live && (pk_bits(over) & (pair ? liveB : liveA)) != 0u) != 0) {   // out-of-range quantised values: exact general reduction
#pragma unroll
                for (uint32_t i = 0; i < 9; ++i) {
                    const uint32_t lo = h[i].x, hi = h[i].y;
                    c[i] = (i % 3 == 0) ? u16x2{(uint16_t)red_y(lo), (uint16_t)red_y(hi)} : u16x2{(uint16_t)red_c(lo), (uint16_t)red_c(hi)};
                }
            }
            px3x2_to_sym13x8<SC>(c, pair ? sB : sA);
        }
        }
        // 16-bit pieces of the 52 output bytes (low half: first triple of the pair, high half: second):
        //   E_j = (s_2j, s_2j+1) of triples 0/2;  O_j = (s_2j+1, s_2j+2) of triples 1/3;  X = (s_12 of 0/2, s_0 of 1/3)
        uint32_t E[6], O[6];
#pragma unroll
        for (uint32_t j = 0; j < 6; ++j) {
            E[j] = pk_bits(sA[2 * j]) | (pk_bits(sA[2 * j + 1]) << 8);
            O[j] = pk_bits(sB[2 * j + 1]) | (pk_bits(sB[2 * j + 2]) << 8);
        }
        const uint32_t X = pk_bits(sA[12]) | (pk_bits(sB[0]) << 8);
        constexpr uint32_t LL = 0x05040100u, HH = 0x07060302u, LH = 0x07060100u;   // v_perm(S0, S1): result = (S1.lo|S0.lo), (S1.hi|S0.hi), (S1.lo|S0.hi)
        uint32_t o[13];
        o[0] = __builtin_amdgcn_perm(E[1], E[0], LL);  o[1] = __builtin_amdgcn_perm(E[3], E[2], LL);  o[2] = __builtin_amdgcn_perm(E[5], E[4], LL);
        o[3] = __builtin_amdgcn_perm(O[0], X, LL);     o[4] = __builtin_amdgcn_perm(O[2], O[1], LL);  o[5] = __builtin_amdgcn_perm(O[4], O[3], LL);
        o[6] = __builtin_amdgcn_perm(E[0], O[5], LH);
        o[7] = __builtin_amdgcn_perm(E[2], E[1], HH);  o[8] = __builtin_amdgcn_perm(E[4], E[3], HH);  o[9] = __builtin_amdgcn_perm(X, E[5], HH);
        o[10] = __builtin_amdgcn_perm(O[1], O[0], HH); o[11] = __builtin_amdgcn_perm(O[3], O[2], HH); o[12] = __builtin_amdgcn_perm(O[5], O[4], HH);
        if constexpr (!IL) {
            if (live) {
                const uint32_t dst = a.sym_off + 13u * t - S0;                    // dword aligned; may sit below sym_off (front slack)
#pragma unroll
                for (uint32_t j = 0; j < 6; ++j) *T3_LDS(u32x2a4, dst + 8u * j) = u32x2a4{o[2 * j], o[2 * j + 1]};
                *T3_LDS(uint32_t, dst + 48u) = o[12];
            }
        } else if (placed) {
            const uint32_t lo = ri == 0u ? r0.lo : ri == 1u ? r1.lo : r2.lo, hi = ri == 0u ? r0.hi : ri == 1u ? r1.hi : r2.hi;
            const uint32_t u0 = 13u * t, dst = (ri == 0u ? r0.dst0 : ri == 1u ? r1.dst0 : r2.dst0) + u0;     // dword aligned
            const bool inside = live && u0 >= lo && u0 + 52u <= hi;
            if (inside) {
#pragma unroll
                for (uint32_t j = 0; j < 6; ++j) *T3_LDS(u32x2a4, dst + 8u * j) = u32x2a4{o[2 * j], o[2 * j + 1]};
                *T3_LDS(uint32_t, dst + 48u) = o[12];
            }
            if (__builtin_amdgcn_ballot_w64(live && !inside) != 0) {              // the few lane units a run's ends cut through: dword by dword
                if (live && !inside) {
#pragma unroll
                    for (uint32_t j = 0; j < 13; ++j) { const uint32_t u = u0 + 4u * j; if (u >= lo && u < hi) *T3_LDS(uint32_t, dst + 4u * j) = o[j]; }
                }
            }
        } else if (live) {
            // 2-D boustrophedon folded into the stores (OLD:750-780): with rows, chunks and the tile start multiples of 4 an aligned
            // dword of the stream stays an aligned dword -- in place in even rows, byte-reversed at the mirrored column in odd
            // rows; any other geometry (and the stream's last, shorter row) goes symbol by symbol
            const uint32_t u0 = 13u * t, lim = 13u * t_end;                       // u0: a multiple of 4; symbols from lim on were never converted
            const bool rows4 = (a.il_w & 3u) == 0u && ((a.il_A & 3u) == 0u || a.il_A >= a.n_sym) && (S0 & 3u) == 0u && (TS & 3u) == 0u;
            IlCursor cur;
            if (u0 < a.n_sym) cur.init(u0, a);
            if (rows4) {
#pragma unroll
                for (uint32_t j = 0; j < 13; ++j) {
                    const uint32_t u = u0 + 4u * j;
                    uint32_t v = u, val = o[j];
                    bool whole = u + 4u <= lim;
                    if (u < a.n_sym) {
                        whole = whole && u + 4u <= a.n_sym && cur.rowlen == a.il_w;
                        if (cur.odd) { v = cur.base + cur.rw + (a.il_w - 4u - cur.c); val = __builtin_bswap32(val); }
                        cur.next(a, 4u);
                    }
                    if (whole) { if (v - S0 < TS) *T3_LDS(uint32_t, a.sym_off + (v - S0)) = val; }
                    else if (u < lim) {
#pragma unroll
                        for (uint32_t i = 0; i < 4; ++i) {
                            const uint32_t uu = u + i, vv = uu < a.n_sym ? il_perm(uu, a) : uu;
                            if (uu < lim && vv - S0 < TS) *T3_LDS(uint8_t, a.sym_off + (vv - S0)) = (uint8_t)(o[j] >> (8u * i));
                        }
                    }
                }
            } else {
#pragma unroll
                for (uint32_t j = 0; j < 13; ++j) {                              // (unrolled: o[] must stay in registers)
#pragma unroll
                    for (uint32_t i = 0; i < 4; ++i) {
                        const uint32_t u = u0 + 4u * j + i;
                        uint32_t v = u;
                        if (u < a.n_sym) { v = cur.get(); cur.next(a); }
                        if (u < lim && v - S0 < TS) *T3_LDS(uint8_t, a.sym_off + (v - S0)) = (uint8_t)(o[j] >> (8u * i));
                    }
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------
// Phase 1 for raw words, packed (1-D; the reference's own entry encode_profile_from_raw OLD:1043, regroup OLD:1051-1082): 3 words = 27
// symbol bytes of which trit 26 of every word is dropped = 78 trits = 26 symbols.  One lane = FOUR word triples = 108 input bytes =
// 27 aligned dwords -> 104 symbols = 26 aligned dwords (round 2 gave a lane one group of 6 words through 28 16-bit LDS reads and a
// division per symbol: 0.111 ms per 8K frame against 0.086 for pixels).  With c[0..26] the triple's bytes:
//   s[m] = c[m]                                  m < 8            (word 0 as it is)
//   s[m] = H(c[m]) + W Lo(c[m+1])                m = 8 .. 25      (word 1 shifted by one trit, word 2 by two)
//     m = 8: c%9 + 9 (c'%3);  9..16: c/3 + 9 (c'%3);  17: (c/3)%3 + 3 (c'%9);  18..25: c/9 + 3 (c'%9)
// computed on pairs (c[8+2i], c[9+2i]) in the 16-bit halves of a register (v_pk_*): H and Lo are element-wise, the pairing of
// Lo(c[m+1]) with H(c[m]) is one v_alignbit per output pair.  Triples are written whole (slack either side of the symbol buffer:
// kSymSlackW); the stage buffer holds real input for all four triples of every live lane (stage_tile rounds up), so stale bytes
// never enter the range check.  Symbols are stored pre-scaled by 2^SH like the pixel converter's.
// ---------------------------------------------------------------------------------------------------------
struct W1Run { uint32_t t_base, t_end, n_units, src0; };      // word triples [t_base, t_end), lane units of four; triple t reads its 27 bytes at src0 + 27 t
__device__ __forceinline__ W1Run w1_run(uint32_t u_lo, uint32_t u_hi, uint32_t stage) {
    W1Run r; r.t_base = (u_lo / 26u) & ~3u; r.t_end = (u_hi + 25u) / 26u; r.n_units = (r.t_end - r.t_base + 3u) / 4u;
    const uint64_t b0 = ((uint64_t)(r.t_base / 2u) * kGroupBytesW) & ~15ull;              // 16-aligned start of the first lane group (two triples each): stage_input
    r.src0 = stage - (uint32_t)b0;                                                         // (wraps; src0 + 27 t does not)
    return r;
}
// A lane unit's two halves (two triples each) go to two different waves -- even converting waves take half 0, odd ones half 1, so the
// byte selectors stay compile-time constants -- which halves the length of phase 1, a serial section of the tile (a wave alone issues a
// vector instruction every four to five cycles).
template <int SH, uint32_t HALF>
__device__ __forceinline__ void convert_words_half(const EncArgs& a, const W1Run r, uint32_t S0, uint32_t lane, uint32_t uw, uint32_t nuw) {
    for (uint32_t e0 = uw * 64u; e0 < r.n_units; e0 += nuw * 64u) {
        const uint32_t e = e0 + lane;
        const uint32_t t = r.t_base + 4u * e;
        const bool live = t < r.t_end;
        const uint32_t src = r.src0 + 27u * (live ? t : r.t_base);                          // dword aligned
        const uint32_t dst = a.sym_off + 26u * t - S0;                                       // dword aligned; may sit below sym_off (front slack)
        {                                                                                    // two triples = 54 bytes in, 52 symbols = 13 dwords out
            constexpr uint32_t half = HALF;
            constexpr uint32_t kDw = 14;
            const uint32_t w0b = 54u * half, d0 = w0b >> 2, B0 = w0b & 3u;                    // the half's bytes start B0 bytes into its first dword
            uint32_t D[kDw];
#pragma unroll
            for (uint32_t i = 0; i < kDw / 2; ++i) { const u32x2a4 v = *T3_LDS(const u32x2a4, src + 4u * d0 + 8u * i); D[2 * i] = v.x; D[2 * i + 1] = v.y; }
            // any byte >= 27?  (b + 101) sets bit 7 exactly for b in 27..154, a byte >= 155 has it set already (a carry only adds set bits).
            // The 56 bytes read hold the half's 54 and two of its neighbours: real input as well (stage_tile stages whole lanes).
            uint32_t hi = 0;
#pragma unroll
            for (uint32_t i = 0; i < kDw; ++i) hi |= D[i] | (D[i] + 0x65656565u);
            if (__builtin_amdgcn_ballot_w64(live && (hi & 0x80808080u) != 0u) != 0) {       // non-canonical symbols: unpack3 reduces every digit (OLD:28-31)
#pragma unroll
                for (uint32_t i = 0; i < kDw; ++i) {
                    uint32_t o = 0;
#pragma unroll
                    for (uint32_t q = 0; q < 4; ++q) { const uint32_t c = (D[i] >> (8u * q)) & 0xFFu; o |= mod27(c) << (8u * q); }   // c < 256 < 512
                    D[i] = o;
                }
            }
            uint32_t R[2][7];
#pragma unroll
            for (uint32_t jj = 0; jj < 2; ++jj) {
                const uint32_t B = B0 + 27u * jj;                                            // first byte of the triple in D
                // byte k of D as the low / high half of a pair (v_perm(S0, S1): selector 0..3 = bytes of S1, 4..7 = of S0, 0x0c = zero)
                auto pair = [&](uint32_t k1, uint32_t k2) -> u16x2 {
                    const uint32_t sel = (k1 & 3u) | 0x0c00u | ((4u + (k2 & 3u)) << 16) | 0x0c000000u;
                    return __builtin_bit_cast(u16x2, __builtin_amdgcn_perm(D[k2 >> 2], D[k1 >> 2], sel));
                };
                u16x2 P[10], Lo[10], H[9];
#pragma unroll
                for (uint32_t m = 0; m < 10; ++m) P[m] = m < 9u ? pair(B + 8u + 2u * m, B + 9u + 2u * m) : __builtin_bit_cast(u16x2, (D[(B + 26u) >> 2] >> (8u * ((B + 26u) & 3u))) & 0xFFu);
                u16x2 q3[5], q9a, q9b;
#pragma unroll
                for (uint32_t m = 0; m < 5; ++m) { q3[m] = pk_d3(P[m]); Lo[m] = P[m] - q3[m] * (uint16_t)3; }     // c % 3 (the low half of Lo[0] is not used)
                q9a = pk_d9(P[0]); q9b = pk_d9(P[4]);
                {   // H[0] = (c8 % 9, c9 / 3)
                    const u16x2 r9 = P[0] - q9a * (uint16_t)9;
                    H[0] = __builtin_bit_cast(u16x2, __builtin_amdgcn_perm(pk_bits(q3[0]), pk_bits(r9), 0x07060100u));
                }
#pragma unroll
                for (uint32_t m = 1; m < 4; ++m) H[m] = q3[m];
                H[4] = q3[4] - q9b * u16x2{0, 3};                                            // (c16 / 3, (c17 / 3) % 3)
#pragma unroll
                for (uint32_t m = 5; m < 10; ++m) { const u16x2 q9 = pk_d9(P[m]); if (m < 9u) H[m] = q9; Lo[m] = P[m] - q9 * (uint16_t)9; }   // c / 9, c % 9
                uint32_t O[9];
#pragma unroll
                for (uint32_t m = 0; m < 9; ++m) {
                    const u16x2 nx = __builtin_bit_cast(u16x2, __builtin_amdgcn_alignbit(pk_bits(Lo[m + 1]), pk_bits(Lo[m]), 16u));   // (Lo of c[9+2m], Lo of c[10+2m])
                    const u16x2 Wv = m < 4u ? u16x2{9, 9} : m == 4u ? u16x2{9, 3} : u16x2{3, 3};
                    O[m] = pk_bits(H[m] + nx * Wv);
                }
                // bytes: s0..s7 = c0..c7, then the nine pairs
                auto dw = [&](uint32_t k) -> uint32_t { return (k & 3u) == 0u ? D[k >> 2] : __builtin_amdgcn_alignbyte(D[(k >> 2) + 1u], D[k >> 2], k & 3u); };
                R[jj][0] = dw(B); R[jj][1] = dw(B + 4u);
#pragma unroll
                for (uint32_t i = 0; i < 4; ++i) R[jj][2 + i] = __builtin_amdgcn_perm(O[2 * i + 1], O[2 * i], 0x06040200u);
                R[jj][6] = __builtin_amdgcn_perm(0u, O[8], 0x0c0c0200u);
#pragma unroll
                for (uint32_t i = 0; i < 7; ++i) R[jj][i] <<= (uint32_t)SH;                   // table-entry offsets (symbols <= 26: no carry between bytes)
            }
            // 52 bytes: the first triple's 26, then the second's at byte 26 (two bytes into dword 6)
            uint32_t o[13];
#pragma unroll
            for (uint32_t i = 0; i < 6; ++i) o[i] = R[0][i];
            o[6] = R[0][6] | (R[1][0] << 16);
#pragma unroll
            for (uint32_t i = 0; i < 6; ++i) o[7 + i] = __builtin_amdgcn_alignbit(R[1][i + 1], R[1][i], 16u);
            if (live) {
                const uint32_t d = dst + 52u * half;
#pragma unroll
                for (uint32_t i = 0; i < 6; ++i) *T3_LDS(u32x2a4, d + 8u * i) = u32x2a4{o[2 * i], o[2 * i + 1]};
                *T3_LDS(uint32_t, d + 48u) = o[12];
            }
        }
    }
}
template <int SH>
__device__ __forceinline__ void convert_words_packed(const EncArgs& a, const W1Run r, uint32_t S0, uint32_t lane, uint32_t wave, uint32_t nwv) {
    const uint32_t nuw = min(a.p1_wpp, nwv / 2u);                                            // waves per half (planner: just enough lane units)
    if (wave >= 2u * nuw) return;
    if (wave & 1u) convert_words_half<SH, 1>(a, r, S0, lane, wave >> 1, nuw); else convert_words_half<SH, 0>(a, r, S0, lane, wave >> 1, nuw);
}

}  // namespace t3
