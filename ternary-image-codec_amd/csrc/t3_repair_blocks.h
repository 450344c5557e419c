// t3_repair_blocks.h — block stages of the FIXED stream repair (t3_repair.hip): where the decoders patch a tile's symbol buffer in LDS
// and keep the data positions only (pos < K, fx2_fix_block), the repair patches the coded bytes in memory, all 26 positions of a block.
//   rp_single        sibling of fx2_single (t3_decode_fx2.h): the single-error closed form, returning (pos, mag) instead of patching LDS
//   rp_patch         one wire byte: received byte mod 27 minus the magnitude.  The scrambler subtracts a state from every trit, so an
//                    additive error on the wire is the same additive error on the descrambled block: nothing is undone
//   rp_canon         bytes 27..255 of an accepted block -> their residue mod 27
//   rp_fix_block     fx2_correct behind the ballot queue -> patches of the wire bytes
//   rp_own_blocks    E1 for the 64 blocks two sets leave with a wave, rp_queue_entry: one queued block
// A lane counts what it changed in RpCount (registers, folded once at the kernel's end).  `write` = T3_REPAIR_WRITE: a dry run counts
// the same and stores nothing.
#pragma once
#include "t3_decode_fx2.h"

namespace t3 {
namespace {

struct RpCount { uint32_t fail, blocks, bytes; };
constexpr uint32_t kRpNonCanon = 1u << 15;           // queue tag bit: the block holds a byte above 26 (tags are < 9 * 24 * 52)

// Single-error closed form for the lane's own block (every position 0..25).  Returns 0: not a single error (-> queue), 1: (pos, mag).
template <int R, uint32_t SMB = 0>
__device__ __forceinline__ uint32_t rp_single(const Synd& sy, uint32_t& pos, uint32_t& mag) {
    constexpr uint32_t SM = SMB + kFx2Small;
    constexpr uint32_t H = R / 2;
    uint32_t lg[R]; bool ok = true;
#pragma unroll
    for (uint32_t j = 0; j < (uint32_t)R; ++j) {
        const uint32_t s = ((j < H ? sy.lo : sy.hi) >> (8u * (j % H))) & 0xFFu;
        lg[j] = lds_u8(SM + kFx2LG + s);
        ok = ok && lg[j] != 0xFFu;
    }
    const uint32_t p = mod26(lg[1] - lg[0]);                                      // S_{j+1} / S_j = alpha^p
#pragma unroll
    for (uint32_t j = 1; j + 1 < (uint32_t)R; ++j) ok = ok && mod26(lg[j + 1] - lg[j]) == p;
    if (!ok) return 0u;
    pos = p; mag = lds_u8(SM + kFx2EX + mod26(lg[0] - p));                        // S_0 = m alpha^p
    return 1u;
}

// one wire byte of an accepted block: y - m = y + 2 m on the received byte mod 27 (always another value than the received one: m != 0)
__device__ __forceinline__ void rp_patch(uint8_t* const p, const uint32_t mag, const uint32_t FMA, const bool write) {
    const uint32_t c = *p, y = c - 27u * div27(c);
    const uint32_t v = lds_u8(FMA + (54u + mag) * 27u + y);
    if (write) *p = (uint8_t)v;
}
// the block's other bytes above 26 (cold: only blocks a wave's ballot flagged); skip: bit i set = position i was patched.  Returns how many.
__device__ __forceinline__ uint32_t rp_canon(uint8_t* const blk, const uint32_t skip, const bool write) {
    uint32_t n = 0;
    for (uint32_t i = 0; i < 26u; ++i) {
        const uint32_t c = blk[i];
        if (c > 26u && !((skip >> i) & 1u)) { if (write) blk[i] = (uint8_t)(c - 27u * div27(c)); ++n; }
    }
    return n;
}
// what an accepted block changed -> the lane's counts
__device__ __forceinline__ void rp_account(RpCount& cn, const uint32_t n) { if (n) { cn.bytes += n; cn.blocks += 1u; } }

// One queued block: syndromes -> corrections patched into the wire bytes at blk.  An uncorrectable block is left as it was received.
template <int R, uint32_t SMB = 0>
__device__ __forceinline__ void rp_fix_block(const uint32_t lo, const uint32_t hi, uint8_t* const blk, const bool noncanon, const uint32_t* __restrict__ root_tbl,
                                             const uint32_t FMA, const bool write, RpCount& cn) {
    constexpr uint32_t H = R / 2;
    uint32_t S[R];
#pragma unroll
    for (uint32_t j = 0; j < (uint32_t)R; ++j) S[j] = ((j < H ? lo : hi) >> (8u * (j % H))) & 0xFFu;
    Fix fx; fx.np = 0;
    if (fx2_correct<R, SMB, true>(S, fx, root_tbl, FMA) != 0u) { cn.fail += 1u; return; }
    uint32_t mask = 0;
#pragma unroll
    for (int q = 0; q < R / 2; ++q)
        if ((uint32_t)q < fx.np) { rp_patch(blk + fx.pos[q], fx.mag[q], FMA, write); mask |= 1u << fx.pos[q]; }
    uint32_t n = fx.np;
    if (noncanon) n += rp_canon(blk, mask, write);
    rp_account(cn, n);
}

// E1 of the repair: clean blocks and single errors are finished by the lane that owns the block, the other flagged blocks appended to the
// queue at q_off (syndromes, 8 bytes; block tags, 2 bytes, behind qcap entries) as fx2_own_blocks does; a block that finds the queue
// full is corrected on the spot.  blkA / blkB: the wire bytes of the lane's block of set A / B; ncA / ncB: that block holds a byte above 26.
template <int R, uint32_t SMB = 0>
__device__ __forceinline__ void rp_own_blocks(const uint32_t* __restrict__ roots, const uint32_t fma_off, const Synd& sA, const Synd& sB, const Blk& bA, const Blk& bB,
                                              uint8_t* const body, const bool ncA, const bool ncB, const uint32_t tag, const uint32_t lane,
                                              const uint32_t cnt_addr, const uint32_t q_off, const uint32_t qcap, const bool write, RpCount& cn) {
    const uint32_t h = lane >> 5;
    Synd own; own.lo = h ? sB.lo : sA.lo; own.hi = h ? sB.hi : sA.hi;
    const bool valid = h ? bB.valid : bA.valid, noncanon = h ? ncB : ncA;
    uint8_t* const blk = body + (h ? bB.off : bA.off);
    bool flagged = valid && (own.lo | own.hi) != 0u;                                // all-zero syndromes: a codeword
    uint32_t pos = 0, mag = 0, single = 0;
    if (flagged) { single = rp_single<R, SMB>(own, pos, mag); flagged = single == 0u; }
    if (valid && !flagged && (single | (noncanon ? 1u : 0u))) {
        uint32_t n = 0, mask = 0;
        if (single) { rp_patch(blk + pos, mag, fma_off, write); mask = 1u << pos; n = 1u; }
        if (noncanon) n += rp_canon(blk, mask, write);
        rp_account(cn, n);
    }
    const uint64_t bal = __builtin_amdgcn_ballot_w64(flagged);
    if (bal != 0ull) {                                                              // wave-aggregated append: one LDS atomic per wave
        const uint32_t cnt = (uint32_t)__popcll(bal), first = (uint32_t)__builtin_ctzll(bal);
        uint32_t base = 0;
        if (__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)) == first) base = __hip_atomic_fetch_add((uint32_t*)__builtin_assume_aligned(lds + cnt_addr, 4), cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        base = __builtin_amdgcn_readlane(base, (int)first);
        if (flagged) {
            const uint32_t slot = base + __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
            if (__builtin_expect(slot < qcap, 1)) {
                *T3_LDS(u32x2, q_off + 8u * slot) = u32x2{own.lo, own.hi};
                *T3_LDS(uint16_t, q_off + 8u * qcap + 2u * slot) = (uint16_t)(tag | (noncanon ? kRpNonCanon : 0u));
            } else rp_fix_block<R, SMB>(own.lo, own.hi, blk, noncanon, roots, fma_off, write, cn);   // queue full (cold)
        }
    }
}

// Queue entry e of tile `tile`: tag = band + 9 K (block within the tile) -> the block's wire bytes
template <int R, uint32_t SMB = 0>
__device__ __forceinline__ void rp_queue_entry(const uint32_t* __restrict__ roots, const uint32_t fma_off, const uint32_t e, const uint32_t q_off, const uint32_t qcap,
                                               uint8_t* const body, const uint32_t tile, const uint32_t nb, const bool write, RpCount& cn) {
    constexpr uint32_t K = 26 - R;
    const u32x2 sy = *T3_LDS(const u32x2, q_off + 8u * e);
    const uint32_t tg = *T3_LDS(const uint16_t, q_off + 8u * qcap + 2u * e);
    const uint32_t yr = tg & (kRpNonCanon - 1u), m = yr / (9u * K), bi = yr - 9u * K * m;
    const uint32_t off = (uint32_t)row(bi).body_off + 26u * (tile * nb + m);
    rp_fix_block<R, SMB>(sy.x, sy.y, body + off, (tg & kRpNonCanon) != 0u, roots, fma_off, write, cn);
}

// ---- the generic kernel's pieces: scrambler state of body symbol i, descramble_symbol OLD:88-94 (a byte above 26 is taken trit-wise) ----
__device__ __forceinline__ uint32_t rp_scr_state(const uint64_t i, const uint32_t cyc24, const uint32_t pre0, const uint32_t pre1) {
    if (i < 2) return i == 0 ? pre0 : pre1;
    return (cyc24 >> (2u * (uint32_t)((i - 2) % 6))) & 3u;
}
__device__ __forceinline__ uint8_t rp_sub_trits(const uint32_t s, const uint32_t st) {
    const uint32_t t0 = (3u + s % 3u - st) % 3u, t1 = (3u + (s / 3u) % 3u - st) % 3u, t2 = (3u + (s / 9u) % 3u - st) % 3u;
    return (uint8_t)(t0 + 3u * t1 + 9u * t2);
}

}  // namespace
}  // namespace t3
