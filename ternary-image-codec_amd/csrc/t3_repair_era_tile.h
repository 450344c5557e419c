// t3_repair_era_tile.h — the block stage of the fused erasure repair kernels, shared by the single-frame kernel (t3_repair_era.hip) and the
// batch kernel (t3_repair_era_frames.hip): GF(27) over the LDS tables in the shape rs_errata asks for, the out-of-line decision of a block
// that holds a byte above 26 (era_block), and rp_own_blocks / rp_queue_entry of t3_repair_blocks.h with the one difference that such a
// block always goes to the queue, tagged.  `body` is the framed body of the tile's own frame.
#pragma once
#include "t3_decode_fx2.h"
#include "t3_repair.h"
#include "t3_repair_blocks.h"
#include "t3_rs_core.h"

namespace t3 {
namespace {
// GF(27) over the fused kernels' LDS tables, in the shape rs_errata asks for: a + x y sits at FMA + 729 x + 27 y + a
struct EraBytes { uint32_t base; __device__ __forceinline__ uint8_t operator[](const int i) const { return (uint8_t)lds_u8(base + (uint32_t)i); } };
struct EraField {
    uint32_t fma; EraBytes neg, inv, exp;
    __device__ __forceinline__ uint8_t M(const uint8_t a, const uint8_t b) const { return (uint8_t)lds_u8(fma + 729u * a + 27u * b); }
    __device__ __forceinline__ uint8_t A(const uint8_t a, const uint8_t b) const { return (uint8_t)lds_u8(fma + 729u + 27u * a + b); }
    __device__ __forceinline__ uint8_t S(const uint8_t a, const uint8_t b) const { return (uint8_t)lds_u8(fma + 1458u + 27u * b + a); }   // a + 2 b
};
struct EraCount { uint32_t flagged, accepted; };
constexpr uint32_t kEraAccepted = 1u << 31;

// One block that holds a byte above 26: mask from its wire bytes, decision from the syndromes (formed with the bytes mod 27 in the erased
// places), corrections patched into the wire bytes.  Returns kEraAccepted | bytes changed, or 0: refused, nothing stored.
template <int R>
__device__ __noinline__ uint32_t era_block(uint8_t* const blk, const uint32_t lo, const uint32_t hi, const uint32_t FMA, const uint32_t write) {
    constexpr uint32_t H = R / 2, SM = kFx2Small;
    uint32_t mask = 0;
    for (uint32_t i = 0; i < 26u; ++i) mask |= (blk[i] > 26u ? 1u : 0u) << i;
    if ((uint32_t)__popc(mask) > (uint32_t)R) return 0u;
    uint8_t S[R], pos[R], mag[R];
#pragma unroll
    for (uint32_t j = 0; j < (uint32_t)R; ++j) S[j] = (uint8_t)(((j < H ? lo : hi) >> (8u * (j % H))) & 0xFFu);
    const EraField g{FMA, {SM + kFx2NEG}, {SM + kFx2INV}, {SM + kFx2EX}};
    int n = 0;
    if (!rs_errata<R>(g, S, mask, pos, mag, n)) return 0u;
    uint32_t cnt = 0;
    for (int e = 0; e < n; ++e)
        if (((mask >> pos[e]) & 1u) != 0u || mag[e] != 0) { rp_patch(blk + pos[e], mag[e], FMA, write != 0u); ++cnt; }   // an erased byte always changes: it was above 26
    return kEraAccepted | cnt;
}

// a queued (or queue-full) block: tagged -> era_block, else the plain repair's correction
template <int R>
__device__ __forceinline__ void era_finish(const uint32_t lo, const uint32_t hi, uint8_t* const blk, const bool tagged, const uint32_t* __restrict__ roots,
                                           const uint32_t FMA, const bool write, RpCount& cn, EraCount& en) {
    if (!tagged) { rp_fix_block<R>(lo, hi, blk, false, roots, FMA, write, cn); return; }
#ifdef T3_ABL_ERA_NO_CHAIN
    en.flagged += 1u; cn.fail += 1u; return;            // timing-only ablation: no out-of-line call in the tile loop (wrong results)
#endif
    const uint32_t r = era_block<R>(blk, lo, hi, FMA, write ? 1u : 0u);
    en.flagged += 1u;
    if (r & kEraAccepted) { en.accepted += 1u; rp_account(cn, r & 0xFFu); } else cn.fail += 1u;
}

// rp_own_blocks with the one difference: a block with a byte above 26 always goes to the queue, tagged
template <int R>
__device__ __forceinline__ void era_own_blocks(const uint32_t* __restrict__ roots, const uint32_t fma_off, const Synd& sA, const Synd& sB, const Blk& bA, const Blk& bB,
                                               uint8_t* const body, const bool ncA, const bool ncB, const uint32_t tag, const uint32_t lane,
                                               const uint32_t cnt_addr, const uint32_t q_off, const uint32_t qcap, const bool write, RpCount& cn, EraCount& en) {
    const uint32_t h = lane >> 5;
    Synd own; own.lo = h ? sB.lo : sA.lo; own.hi = h ? sB.hi : sA.hi;
    const bool valid = h ? bB.valid : bA.valid, tagged = valid && (h ? ncB : ncA);
    uint8_t* const blk = body + (h ? bB.off : bA.off);
    bool flagged = valid && ((own.lo | own.hi) != 0u || tagged);
    if (flagged && !tagged) {
        uint32_t pos = 0, mag = 0;
        if (rp_single<R>(own, pos, mag) != 0u) { rp_patch(blk + pos, mag, fma_off, write); rp_account(cn, 1u); flagged = false; }
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
                *T3_LDS(uint16_t, q_off + 8u * qcap + 2u * slot) = (uint16_t)(tag | (tagged ? kRpNonCanon : 0u));
            } else era_finish<R>(own.lo, own.hi, blk, tagged, roots, fma_off, write, cn, en);   // queue full (never: 9 x 52 <= 512)
        }
    }
}

template <int R>
__device__ __forceinline__ void era_queue_entry(const uint32_t* __restrict__ roots, const uint32_t fma_off, const uint32_t e, const uint32_t q_off, const uint32_t qcap,
                                                uint8_t* const body, const uint32_t tile, const uint32_t nb, const bool write, RpCount& cn, EraCount& en) {
    constexpr uint32_t K = 26 - R;
    const u32x2 sy = *T3_LDS(const u32x2, q_off + 8u * e);
    const uint32_t tg = *T3_LDS(const uint16_t, q_off + 8u * qcap + 2u * e);
    const uint32_t yr = tg & (kRpNonCanon - 1u), m = yr / (9u * K), bi = yr - 9u * K * m;
    const uint32_t off = (uint32_t)row(bi).body_off + 26u * (tile * nb + m);
    era_finish<R>(sy.x, sy.y, body + off, (tg & kRpNonCanon) != 0u, roots, fma_off, write, cn, en);
}
}  // namespace
}  // namespace t3
