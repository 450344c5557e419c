// t3_enc_parity.h — phase 2 of the fused encoder (t3_encode.h): RS parity, scrambling and the band-serial stores of one tile whose
// stream-ordered symbols sit in LDS.  Device-only, header-inline.
//   LDS header rows      BandRow / band_row / band_first
//   LUT path (mixed k)   add13, Blk26, encode_block, phase2_band
//   matrix cores         P2Map, phase2_mfma (v_mfma_i32_32x32x32_i8)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "t3_device.h"
#include "t3_devutil.h"

namespace t3 {

constexpr uint32_t kEncChunk = 5;      // data symbols whose LUT reads may be in flight together
template <int R> struct LutGeo { static constexpr uint32_t SLAB = lut_slab_bytes(R), VOFF = lut_var_off(R); };     // lut_geom()'s, t3_device.h

struct Blk26 { uint32_t w[7]; };   // 26 output bytes, little-endian packed (w[6] holds 2)
struct BandRow { uint32_t k, nbt, blocks, lut_off, pad_, boff6; uint64_t body_off; };   // LDS header row b
static_assert(sizeof(BandRow) == kHdrBandRow, "BandRow is one header row");
__device__ __forceinline__ BandRow band_row(uint32_t b) { return *(const BandRow*)(lds + (uint32_t)kHdrBandRow * b); }
__device__ __forceinline__ uint32_t band_first(uint32_t b) { return *(const uint32_t*)(lds + (uint32_t)kHdrBandFirst + 4u * b); }

__device__ __forceinline__ uint32_t add13(uint32_t d, uint32_t s) {   // d + (s,s,s) trit-wise (scramble_symbol OLD:81-87)
    const uint32_t q1 = div3(d), q2 = div9(d);
    uint32_t t0 = d - 3u * q1 + s, t1 = q1 - 3u * q2 + s, t2 = q2 + s;
    t0 -= t0 >= 3u ? 3u : 0u; t1 -= t1 >= 3u ? 3u : 0u; t2 -= t2 >= 3u ? 3u : 0u;
    return t0 + 3u * t1 + 9u * t2;
}

// One RS block.  The stream-ordered LDS symbol buffer holds symbols PRE-SCALED by 8 (= the byte offset of the symbol's
// 8-byte LUT entry), so a data symbol costs: one ds_read_u8, then per table one ds_read_b64/b32 whose address is that
// byte plus an immediate — no address arithmetic for the fixed tables.  Parity contributions arrive as 6-bit SWAR trit
// fields (5 per dword; k*2+2 <= 50 < 64, no carries) and are folded mod 3 once per block.  The table that carries the
// last accumulator dword exists in three variants, one per scrambler state, and holds the scrambled image of the symbol
// in its top byte: choosing the variant (one add of a per-lane class base) scrambles, one v_perm_b32 places the byte.
//   sym_addr : LDS byte address of the block's first data symbol;  lut: LDS byte address of the band's LUT
//   c0       : scrambler cycle phase of the block's first body symbol ((i0 - 2) mod 6)
//   first    : block starts at body symbol 0 (the two pre-period states apply)
template <int R, bool FIXED_LUT>
__device__ __forceinline__ Blk26 encode_block(uint32_t sym_addr, uint32_t lut_rt, uint32_t c0, bool first, const EncArgs& a) {
    constexpr uint32_t K = 26 - R;
    using G = LutGeo<R>;
    const uint32_t lut = FIXED_LUT ? (uint32_t)kLdsHdr : lut_rt;       // single-k launches: LUT sits right behind the header
    uint32_t st[6], vb[6];                          // scrambler state per residue class of the position (6-periodic)
#pragma unroll
    for (int q = 0; q < 6; ++q) {
        st[q] = (a.cyc24 >> (2u * (c0 + q))) & 3u;
        vb[q] = (FIXED_LUT ? 0u : lut) + (st[q] << 8);                   // variant tables are 256 B apart
    }
    uint32_t acc0 = 0, acc1 = 0, acc2 = 0, acc3 = 0, acc4 = 0;
    Blk26 o;
#pragma unroll
    for (int i = 0; i < 7; ++i) o.w[i] = 0;
    uint32_t d0 = 0, d1 = 0;
#pragma unroll
    for (uint32_t p = 0; p < K; ++p) {
        const uint32_t d8 = lds[sym_addr + 9u * p];
        if (p == 0) d0 = d8;
        if (p == 1) d1 = d8;
        const uint32_t fa = FIXED_LUT ? d8 : d8 + lut;                   // fixed tables: byte offset + immediate
        const uint2 A = *(const uint2*)(lds + fa + (FIXED_LUT ? lut : 0u) + p * G::SLAB);
        acc0 += A.x; acc1 += A.y;
        if constexpr (R == 8) { const uint2 B = *(const uint2*)(lds + fa + (FIXED_LUT ? lut : 0u) + p * G::SLAB + 256u); acc2 += B.x; acc3 += B.y; }
        const uint32_t va = d8 + vb[p % 6];
        uint32_t img;
        if constexpr (R == 6) {
            const uint2 V = *(const uint2*)(lds + va + (FIXED_LUT ? lut : 0u) + p * G::SLAB + G::VOFF);
            acc2 += V.x; acc3 += V.y; img = V.y;
        } else {
            const uint32_t V = *(const uint32_t*)(lds + va + (FIXED_LUT ? lut : 0u) + p * G::SLAB + G::VOFF);
            if constexpr (R == 8) acc4 += V; else acc2 += V;
            img = V;
        }
        // result byte (p&3) <- top byte of img, other bytes kept
        constexpr uint32_t sel[4] = {0x03020107u, 0x03020700u, 0x03070100u, 0x07020100u};
        o.w[p >> 2] = __builtin_amdgcn_perm(img, o.w[p >> 2], sel[p & 3]);
        if (p % kEncChunk == kEncChunk - 1) {
            // bound the LUT reads in flight: without this the compiler issues all reads first and sinks the adds (spills)
            asm volatile("" : "+v"(acc0), "+v"(acc1), "+v"(acc2), "+v"(acc3), "+v"(acc4), "+v"(o.w[p >> 2]));
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    // parity symbols get their own scrambler states: add them to the trit fields before the mod-3 fold
    constexpr int NMAIN = R < 5 ? R : 5;
    uint32_t cm = 0;
#pragma unroll
    for (int j = 0; j < NMAIN; ++j) cm |= st[(K + j) % 6] << (6 * j);
    const uint32_t x0 = mod3x5(acc0 + cm), x1 = mod3x5(acc1 + cm), x2 = mod3x5(acc2 + cm);
    const uint32_t S = x0 + 3u * x1 + 9u * x2;           // five parity symbols in 6-bit fields
    uint32_t par[8];
#pragma unroll
    for (int j = 0; j < NMAIN; ++j) par[j] = (S >> (6 * j)) & 63u;
    if constexpr (R == 6) {
        const uint32_t x3 = mod3x5(acc3 + st[(K + 5) % 6] * 0x1041u);
        par[5] = (x3 & 63u) + 3u * ((x3 >> 6) & 63u) + 9u * ((x3 >> 12) & 63u);
    }
    if constexpr (R == 8) {
        const uint32_t s5 = st[(K + 5) % 6], s6 = st[(K + 6) % 6], s7 = st[(K + 7) % 6];
        const uint32_t x3 = mod3x5(acc3 + s5 * 0x1041u + s6 * 0x1040000u);
        const uint32_t x4 = mod3x5(acc4 + s6 + s7 * 0x41040u);
        par[5] = (x3 & 63u) + 3u * ((x3 >> 6) & 63u) + 9u * ((x3 >> 12) & 63u);
        par[6] = ((x3 >> 18) & 63u) + 3u * ((x3 >> 24) & 63u) + 9u * (x4 & 63u);
        par[7] = ((x4 >> 6) & 63u) + 3u * ((x4 >> 12) & 63u) + 9u * ((x4 >> 18) & 63u);
    }
#pragma unroll
    for (int j = 0; j < R; ++j) { const int p = K + j; o.w[p >> 2] |= par[j] << (8 * (p & 3)); }
    if (first)   // body symbols 0 and 1 see the pre-period states (exact whatever the seed; OLD:81-87)
        o.w[0] = (o.w[0] & 0xFFFF0000u) | add13(d0 >> 3, a.pre0) | (add13(d1 >> 3, a.pre1) << 8);
    return o;
}

// Phase 2 for one lane: encode block m of band b and store its 26 bytes straight to the band's run in global memory.
// A block starts 2-byte aligned (header and band offsets are even), so it is exactly six aligned dwords plus one short —
// at the front when the block starts at 2 (mod 4), at the back otherwise: 7 stores per lane, no overlap with the
// neighbour blocks, no LDS staging.  Consecutive lanes hold consecutive blocks, so a wave's seven store instructions
// cover one contiguous 1664-byte run (13 cache lines).
template <int R, bool FIXED_LUT>
__device__ __forceinline__ bool phase2_band(const EncArgs& a, uint32_t symb, uint32_t tile, uint32_t b, uint32_t m, uint32_t nbt) {
    constexpr uint32_t K = 26 - R;
    const uint32_t mg = tile * nbt + m;
    const BandRow r = band_row(b);
    if (!(m < nbt && mg < r.blocks)) return false;
    const uint32_t c0 = (r.boff6 + 2u * (mg % 3u)) % 6u;                             // 26 == 2 (mod 6)
    const Blk26 o = encode_block<R, FIXED_LUT>(symb + b + 9u * K * m, r.lut_off, c0, r.body_off == 0 && mg == 0, a);
    uint8_t* G = a.body_out + r.body_off + 26ull * mg;
    const bool al = ((uint32_t)(uintptr_t)G & 2u) == 0;
    uint32_t* base = (uint32_t*)(G + (al ? 0 : 2));                                    // six aligned dwords
#pragma unroll
    for (int i = 0; i < 6; ++i) base[i] = al ? o.w[i] : ((o.w[i] >> 16) | (o.w[i + 1] << 16));
    *(uint16_t*)(G + (al ? 24 : 0)) = (uint16_t)(al ? o.w[6] : o.w[0]);                // and the remaining short
    return true;
}

// ---------------------------------------------------------------------------------------------------------
// Phase 2 on the matrix cores (single-k launches).  RS parity is GF(3)-linear in the data trits: per block a (3r x 3k)
// matrix-vector product mod 3.  One v_mfma_i32_32x32x32_i8 chain (3 K-steps) does it for 32 blocks: the B operand is the
// data, one dword per symbol = its three trits as bytes (byte 3 carries the scrambled symbol and meets a zero matrix
// column), fetched from a 27-entry LDS table per scrambler state; lane (n, h) supplies positions 8s + 4h + d of block n in
// K-step s.  The A operand (the matrix, host-built in the instruction's lane order) sits in 12 VGPRs.  The accumulators
// come back as: lane (n, h) holds the three trit sums of parity symbols h r/2 .. h r/2 + r/2 - 1 of block n; adding the
// scrambler state and folding mod 3 is three byte-table reads per symbol.  A wave does two sets of 32 blocks.
// Output: lane (n, h) owns bytes [8s + 4h, +4) of the block for s = 0..2 (plus bytes 24, 25 for h = 1): three dword
// stores at 2-byte alignment and one short.  Returns the number of global store instructions issued (wave-uniform).
// ---------------------------------------------------------------------------------------------------------

struct __attribute__((packed, aligned(1))) U128a1 { uint32_t v[4]; };

// How the (up to) two sets of a call map to blocks: set s covers items item0[s] .. item0[s] + 31 of a run of n_items blocks
// dealt linearly over bands that share k: item -> (band index item / nb, block item % nb); band_tab = LDS address of the
// index -> band bytes (UEP groups) or ~0 for the identity (one k on all nine bands).
struct P2Map { uint32_t item0[2]; uint32_t n_items, nb; DevDiv div_nb; uint32_t band_tab, scr_off; };

template <int R, bool GRP, bool BCN, bool REGEO = false>      // BCN: beacon insertion fused into the stores; GRP: UEP group call (one set, band table, the group's scrambler dwords); else one k on all nine bands (two sets); REGEO: see load()
__device__ __forceinline__ uint32_t phase2_mfma(const EncArgs& a, uint32_t symb, uint32_t tile, uint32_t lane, const v4i (&Afr)[3], const P2Map& M, const uint64_t out_base = 0) {   // out_base: the frame's byte offset from a.body_out (batch launches)
    constexpr uint32_t K = 26 - R, H = R / 2;
    constexpr uint32_t TB = GRP ? kLdsHdrUep : kLdsHdr, MB = TB + kMfmaModOff;
    const uint32_t n = lane & 31u, h = lane >> 5;
    const uint32_t tb3 = __builtin_amdgcn_readfirstlane((tile * M.nb) % 3u);
    // A wave does two sets of 32 blocks.  The table reads of BOTH sets are issued before either set's MFMA chain, so the
    // second set's two dependent LDS round trips hide under the first set's chain and epilogue.
    struct Set { v4i Bv[3]; uint32_t W[3]; uint32_t c0, mg; uint64_t goff; bool valid, first; uint32_t dd0, dd1; };
    auto load = [&](uint32_t set, Set& s) {
        uint32_t nn = n;
        if constexpr (REGEO) asm volatile("" : "+v"(nn));                     // the wave's items never change: hoisted out of the tile loop, both sets' block geometry was kept in (spilled)
                                                                              // registers by the kernels that are over the 80-VGPR budget (reloads + vmcnt(0) in every tile): those recompute it
        const uint32_t item = M.item0[set] + nn;                              // blocks are dealt linearly across the bands (item0 huge: no set)
        const uint32_t bi = min(div_any(item, M.div_nb), 8u), m = item - bi * M.nb;
        uint32_t b = bi;
        if constexpr (GRP) b = lds_u8(M.band_tab + bi);
        const BandRow r = band_row(b);
        s.mg = tile * M.nb + m;
        s.valid = item < M.n_items && s.mg < r.blocks;                        // lanes without a block run along (reads stay inside LDS) and store nothing
        s.goff = r.body_off + 26ull * s.mg;
        s.first = r.body_off == 0 && s.mg == 0 && h == 0;
        // scrambler phase of the block's first symbol: (boff6 + 2 (mg mod 3)) mod 6 (26 == 2 mod 6), without wide multiplies
        uint32_t m3 = tb3 + m - 3u * ((m * 683u) >> 11); m3 -= m3 >= 3u ? 3u : 0u;   // m < 2048
        uint32_t c0 = r.boff6 + 2u * m3; c0 -= c0 >= 6u ? 6u : 0u;
        s.c0 = c0;
        uint32_t c0h = c0 + 4u * h; c0h -= c0h >= 6u ? 6u : 0u;               // ... of this lane's first position 4h
        const uint32_t cycs = a.cyc24 >> (2u * c0h);
        uint32_t vb[6];                                                       // table base per position class: state (4 KiB apart), own bank copy
#pragma unroll
        for (uint32_t q = 0; q < 6; ++q) vb[q] = (((cycs >> (2u * q)) & 3u) << 12) | (TB + 4u * n);
        const uint32_t sa = symb + b + 9u * K * m + 36u * h;
        s.dd0 = 0; s.dd1 = 0;
#pragma unroll
        for (uint32_t st = 0; st < 3; ++st) {
            uint32_t x[4];
#pragma unroll
            for (uint32_t d = 0; d < 4; ++d) {
                const uint32_t d4 = lds_u8(sa + 72u * st + 9u * d);           // positions >= k read neighbouring bytes: they meet zero matrix columns
                if (set == 0 && st == 0 && d == 0) s.dd0 = d4;                // (body symbols 0 and 1 sit in set 0 of wave 0)
                if (set == 0 && st == 0 && d == 1) s.dd1 = d4;
                x[d] = lds_u32((d4 << 5) + vb[(8u * st + d) % 6u]);
                s.Bv[st][d] = (int)x[d];
            }
            const uint32_t t01 = __builtin_amdgcn_perm(x[1], x[0], 0x0c0c0703u), t23 = __builtin_amdgcn_perm(x[3], x[2], 0x07030c0cu);
            s.W[st] = t01 | t23;                                               // the four scrambled symbols
        }
    };
    auto finish = [&](Set& s) -> uint32_t {
        uint32_t c0K = s.c0 + (K % 6u); c0K -= c0K >= 6u ? 6u : 0u;           // scrambler phase of the first parity symbol
        if constexpr (R >= 4) {     // the states of the parity symbols ride in unused positions of the upper half (see mfma_scr_pos)
            const u32x2 sd = *T3_LDS(const u32x2, (GRP ? M.scr_off : (uint32_t)kHdrScr) + 8u * c0K);
            if constexpr (R == 4) s.Bv[2][2] = h ? (int)sd.x : s.Bv[2][2];
            else { s.Bv[2][0] = h ? (int)sd.x : s.Bv[2][0]; s.Bv[2][1] = h ? (int)sd.y : s.Bv[2][1]; }
        }
        v16i acc = {64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64};   // bias: trit sums in [-60, 62] -> table index
#ifndef T3_ABL_NO_MFMA
#pragma unroll
        for (uint32_t st = 0; st < 3; ++st) acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(Afr[st], s.Bv[st], acc, 0, 0, 0);
#else
        acc[0] += s.Bv[0][0] & 1; acc[3] += s.Bv[1][1] & 1; acc[6] += s.Bv[2][2] & 1; acc[1] += (s.Bv[0][1] ^ s.Bv[0][2] ^ s.Bv[0][3] ^ s.Bv[1][0] ^ s.Bv[1][2] ^ s.Bv[1][3] ^ s.Bv[2][0] ^ s.Bv[2][1] ^ s.Bv[2][3]) & 1;
#endif
        // parity symbols of this lane: h H + jj; mod-3 fold and 3^t weight by byte tables (one bank per dword: conflict-free)
        uint32_t Pown = 0;
#pragma unroll
        for (uint32_t jj = 0; jj < H; ++jj) {
            uint32_t x0 = (uint32_t)acc[3 * jj], x1 = (uint32_t)acc[3 * jj + 1], x2 = (uint32_t)acc[3 * jj + 2];
            if constexpr (R == 2) {                                              // k = 24: no free position, add the state here
                const uint32_t stt = (a.cyc24 >> (2u * (c0K + h))) & 3u;
                x0 += stt; x1 += stt; x2 += stt;
            }
            const uint32_t sym = lds_u8(MB + x0) + lds_u8(MB + 128u + x1) + lds_u8(MB + 256u + x2);
            Pown |= sym << (8u * jj);
        }
        const uint32_t Plo = __builtin_amdgcn_permlane32_swap(Pown, Pown, false, false)[0];   // upper half: the h = 0 partner's parities
        uint32_t W2 = s.W[2], tail;
        if constexpr (R == 6)      { W2 = h ? ((Plo & 0x00FFFFFFu) | (Pown << 24)) : W2; tail = Pown >> 8; }
        else if constexpr (R == 8) { W2 = h ? ((Plo >> 16) | (Pown << 16)) : ((W2 & 0xFFFFu) | (Pown << 16)); tail = Pown >> 16; }
        else if constexpr (R == 4) { W2 = h ? ((W2 & 0xFFFFu) | (Plo << 16)) : W2; tail = Pown; }
        else                       { tail = (Plo & 0xFFu) | (Pown << 8); }
        uint32_t W0 = s.W[0];
        if (s.first)                                            // body symbols 0 and 1 see the pre-period states (exact whatever the seed; OLD:81-87)
            W0 = (W0 & 0xFFFF0000u) | add13(s.dd0 >> 2, a.pre0) | (add13(s.dd1 >> 2, a.pre1) << 8);
        // Lane (n, h) holds bytes [8s + 4h, +4) of block n.  Two half-wave exchanges give the lower lane bytes 0..15 and the
        // upper lane bytes 10..25 of the block: ONE 16-byte store per lane covers the 26 bytes (bytes 10..15 are written by
        // both, with the same values), instead of three scattered dwords and a short -- an eighth of the cache-line requests.
        // v_permlane32_swap(a, b): a's upper half-wave <-> b's lower half-wave.  swap(W0, W1) and swap(W1, W2) leave in every lane the
        // four dwords of its 16-byte run in order -- h=0: bytes 0..3, 4..7, 8..11, 12..15; h=1: 8..11, 12..15, 16..19, 20..23 --
        // and one v_perm per dword with a per-lane selector takes them as they are (h=0) or shifted by two bytes (h=1: bytes 10..25).
        const auto q01 = __builtin_amdgcn_permlane32_swap(W0, s.W[1], false, false);
        const auto q23 = __builtin_amdgcn_permlane32_swap(s.W[1], W2, false, false);
        const uint32_t selE = h ? 0x05040302u : 0x03020100u;                      // v_perm(S0, S1): 0..3 = bytes of S1, 4..7 = bytes of S0
        U128a2 E;
        E.v[0] = __builtin_amdgcn_perm(q01[1], q01[0], selE);
        E.v[1] = __builtin_amdgcn_perm(q23[0], q01[1], selE);
        E.v[2] = __builtin_amdgcn_perm(q23[1], q23[0], selE);
        E.v[3] = __builtin_amdgcn_perm(tail, q23[1], selE);                        // h=1: bytes 22..25
        if constexpr (BCN) {
            // The run's 16 body bytes start at body offset g0; nb0 beacons lie in front of it in the framed stream and the next one
            // comes after c more body bytes.  c < 16: it falls inside the run, whose bytes from c on move up by one (the 17th
            // byte goes out on its own); c == bcn_pb with a beacon directly in front of the run (only a block's first run can
            // have no run before it that holds that beacon): this lane writes it.  bcn_pb >= 17: one beacon per run at most.
            const uint32_t g0 = (uint32_t)s.goff + 10u * h;                       // body symbols are 31-bit (plan_layout)
            uint32_t nb0 = 0, c = a.bcn_slot - g0;
            if (g0 >= a.bcn_slot) { const uint32_t u = g0 - a.bcn_slot, j = div_ge2(u, a.bcn_div); nb0 = j + 1u; c = a.bcn_pb - (u - j * a.bcn_pb); }
            const bool inside = c < 16u, pre = nb0 != 0u && c == a.bcn_pb;
            const uint32_t dc = inside ? c >> 2 : 4u, bc = c & 3u;
            const uint32_t Ed = dc == 0u ? E.v[0] : dc == 1u ? E.v[1] : dc == 2u ? E.v[2] : E.v[3];
            const uint32_t sel = bc == 0u ? 0x02010004u : bc == 1u ? 0x02010400u : bc == 2u ? 0x02040100u : 0x04020100u;
            const uint32_t Mx = __builtin_amdgcn_perm(a.bcn_sym, Ed, sel);        // low bc bytes, the beacon, the rest one byte up
            U128a1 F;
            F.v[0] = dc == 0u ? Mx : E.v[0];
#pragma unroll
            for (uint32_t i = 1; i < 4; ++i) F.v[i] = i < dc ? E.v[i] : i == dc ? Mx : __builtin_amdgcn_alignbyte(E.v[i], E.v[i - 1], 3u);
            uint8_t* dst = a.body_out + out_base + (s.goff + 10u * h + nb0);
            const bool extra = s.valid && (inside || pre);
            if (s.valid) *(U128a1*)dst = F;                                         // any byte alignment
            const bool any_extra = __builtin_amdgcn_ballot_w64(extra) != 0;
            if (any_extra) { if (extra) *(inside ? dst + 16 : dst - 1) = (uint8_t)(inside ? E.v[3] >> 24 : a.bcn_sym); }
            return (__builtin_amdgcn_ballot_w64(s.valid) != 0 ? 1u : 0u) + (any_extra ? 1u : 0u);
        }
#ifdef T3_ABL_NO_STORE
        if (s.valid && a.n_tiles == 0xFFFFFFFFu)
#else
        if (s.valid)
#endif
            *(U128a2*)(a.body_out + out_base + s.goff + 10u * h) = E;                         // 2-byte aligned (measured: as fast as 16-byte aligned)
#ifndef T3_ABL_NO_STORE
        return __builtin_amdgcn_ballot_w64(s.valid) != 0 ? 1u : 0u;               // a store with no active lane is branched over
#else
        return 0u;
#endif
    };
    Set s0;
    load(0, s0);
    if constexpr (GRP) return finish(s0);                                    // UEP path: one set per call
    Set s1;
    load(1, s1);
    uint32_t issued = finish(s0);
    issued += finish(s1);
    return issued;
}

}  // namespace t3
