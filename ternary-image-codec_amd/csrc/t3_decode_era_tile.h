// t3_decode_era_tile.h — the block stage of the fused FIXED pixel decoder with received bytes above 26 taken as erasures, shared by
// decode_era_px_kernel (t3_decode_era.hip, one frame) and decode_era_frames_px (t3_decode_era_frames.hip, a batch of equal frames in one
// launch): the LDS words of the counts, the out-of-line errata step of a tagged block, the producers' append and the consumers' queue
// entry.  Each of the two units compiles it and keeps its own tile loop, as the repairs do with t3_repair_era_tile.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "t3_decode.h"
#include "t3_decode_fx.h"
#include "t3_decode_fx2.h"
#include "t3_decode_wg.h"
#include "t3_decode_px.h"
#include "t3_repair.h"
#include "t3_repair_blocks.h"
#include "t3_repair_tile.h"
#include "t3_repair_era_tile.h"
#include "t3_rs_core.h"

namespace t3 {

namespace {
// LDS: decode_fixed_px_kernel's, the queues kEraQCap entries each; counts [1] at kFx2FailWg, [2] and [3] in the header's free words behind
// the band rows
constexpr uint32_t kEraCntFlagged = 144, kEraCntAccepted = 148;
static_assert(9 * T3_DEC_PX_NB <= kEraQCap && 9 * 24 * T3_DEC_PX_NB < (int)kRpNonCanon, "every block of a tile fits the queue, every tag the 15 bits");

// One tagged block: decision from the mask and the queued syndromes (formed with the bytes mod 27 in the erased places), corrections patched
// into the symbol buffer at yb (data positions only).  Returns 1: accepted, 0: refused, nothing stored.
template <int R>
__device__ __noinline__ uint32_t era_px_block(const uint32_t mask, const uint32_t lo, const uint32_t hi, const uint32_t FMA, const uint32_t yb) {
    constexpr uint32_t K = 26 - R, H = R / 2, SM = kFx2Small;
    if ((uint32_t)__popc(mask) > (uint32_t)R) return 0u;
    uint8_t S[R], pos[R], mag[R];
#pragma unroll
    for (uint32_t j = 0; j < (uint32_t)R; ++j) S[j] = (uint8_t)(((j < H ? lo : hi) >> (8u * (j % H))) & 0xFFu);
    const EraField g{FMA, {SM + kFx2NEG}, {SM + kFx2INV}, {SM + kFx2EX}};
    int n = 0;
    if (!rs_errata<R>(g, S, mask, pos, mag, n)) return 0u;
    for (int e = 0; e < n; ++e)
        if ((uint32_t)pos[e] < K && mag[e] != 0) { const uint32_t ad = yb + 9u * pos[e]; *T3_LDS(uint8_t, ad) = (uint8_t)lds_u8(FMA + (54u + mag[e]) * 27u + lds_u8(ad)); }   // y - m = y + 2 m
    return 1u;
}

// fx2_own_blocks with the one difference: a block with a byte above 26 always goes to the queue, tagged (the queue holds every block of a tile)
template <int R>
__device__ __forceinline__ void era_px_own_blocks(const uint32_t fma_off, const Synd& sA, const Synd& sB, const Blk& bA, const Blk& bB, const bool ncA, const bool ncB,
                                                  const uint32_t tag, const uint32_t lane, const uint32_t cnt_addr, const uint32_t q_off) {
    const uint32_t h = lane >> 5;
    Synd own; own.lo = h ? sB.lo : sA.lo; own.hi = h ? sB.hi : sA.hi;
    const bool valid = h ? bB.valid : bA.valid, tagged = valid && (h ? ncB : ncA);
    const uint32_t yb = h ? bB.yb : bA.yb;
    bool flagged = valid && ((own.lo | own.hi) != 0u || tagged);
    if (flagged && !tagged) flagged = fx2_single<R>(own, yb, fma_off) == 0u;
    const uint64_t bal = __builtin_amdgcn_ballot_w64(flagged);
    if (bal != 0ull) {                                                              // wave-aggregated append: one LDS atomic per wave
        const uint32_t cnt = (uint32_t)__popcll(bal), first = (uint32_t)__builtin_ctzll(bal);
        uint32_t base = 0;
        if (__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)) == first) base = __hip_atomic_fetch_add((uint32_t*)__builtin_assume_aligned(lds + cnt_addr, 4), cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        base = __builtin_amdgcn_readlane(base, (int)first);
        if (flagged) {
            const uint32_t slot = base + __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
            if (slot < kEraQCap) {                                                  // (always: the static_assert above)
                *T3_LDS(u32x2, q_off + 8u * slot) = u32x2{own.lo, own.hi};
                *T3_LDS(uint16_t, q_off + 8u * kEraQCap + 2u * slot) = (uint16_t)(tag | (tagged ? kRpNonCanon : 0u));
            }
        }
    }
}

// Queue entry e of tile `tile` (its index inside its frame; body: that frame's): untagged -> fx2_queue_entry's work; tagged -> the mask
// from the block's wire bytes, then era_px_block
template <int R, bool BCN>
__device__ __forceinline__ void era_px_queue_entry(const DecFx2Args& a, const uint8_t* const body, const uint32_t e, const uint32_t q_off, const uint32_t y_off, const uint32_t tile) {
    constexpr uint32_t K = 26 - R;
    const u32x2 sy = *T3_LDS(const u32x2, q_off + 8u * e);
    const uint32_t tg = *T3_LDS(const uint16_t, q_off + 8u * kEraQCap + 2u * e);
    uint32_t* const failp = (uint32_t*)(lds + kFx2FailWg);
    if ((tg & kRpNonCanon) == 0u) { if (!fx2_fix_block<R>(sy.x, sy.y, y_off + tg, a.roots, a.fma_off)) atomicAdd(failp, 1u); return; }
    const uint32_t yr = tg & (kRpNonCanon - 1u), m = yr / (9u * K), bi = yr - 9u * K * m;
    const uint32_t off = (uint32_t)row(bi).body_off + 26u * (tile * a.nb + m);
    uint32_t mask = 0;
    for (uint32_t i = 0; i < 26u; ++i) {
        uint32_t g = off + i;
        if constexpr (BCN) { if (g >= a.bcn_slot) g += div_ge2(g - a.bcn_slot, a.bcn_div) + 1u; }   // the beacons in front of body byte g (load_run)
        mask |= (body[g] > 26u ? 1u : 0u) << i;
    }
    const uint32_t ok = era_px_block<R>(mask, sy.x, sy.y, a.fma_off, y_off + yr);
    atomicAdd((uint32_t*)(lds + kEraCntFlagged), 1u);
    atomicAdd(ok ? (uint32_t*)(lds + kEraCntAccepted) : failp, 1u);
}
}  // namespace

}  // namespace t3
