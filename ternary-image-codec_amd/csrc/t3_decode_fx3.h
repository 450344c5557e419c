// t3_decode_fx3.h — the queued blocks of the RS(26,20) pixel decoders (decode_fixed_px_kernel<6, *, false>, dec_frames_px<6, *, false>):
// E1 has fixed the single errors, so a queued block of a correctable frame carries two or three.  fx2_solve (t3_rs_solve3.h) finds their
// locator from determinants -- about 20 dependent table reads where Berlekamp-Massey + Omega + Forney (fx2_correct) take about 60 -- and
// fx2_correct stays behind a wave-uniform branch for every block the closed form does not decide: only it refuses a block.  Same tables,
// same LDS.  Every other decoder keeps fx2_correct alone.
#pragma once
#include "t3_decode_fx2.h"
#include "t3_rs_solve3.h"

namespace t3 {
namespace {

// the field of fx2_solve on the device: table index of a + x y = FMA + 729 x + 27 y + a (t3_decode_fx2.h)
template <uint32_t SMB>
struct Fx3Lds {
    uint32_t FMA; const uint32_t* __restrict__ root_tbl;
    static constexpr uint32_t SM = SMB + kFx2Small;
    __device__ __forceinline__ uint32_t mad(const uint32_t a, const uint32_t x, const uint32_t y) const { return lds_u8(FMA + __umul24(x, 729u) + __umul24(y, 27u) + a); }
    __device__ __forceinline__ uint32_t neg(const uint32_t x) const { return lds_u8(SM + kFx2NEG + x); }
    __device__ __forceinline__ uint32_t inv(const uint32_t x) const { return lds_u8(SM + kFx2INV + x); }
    __device__ __forceinline__ uint32_t ninv(const uint32_t x) const { return lds_u8(SM + kFx2NINV + x); }
    __device__ __forceinline__ uint32_t ex(const uint32_t i) const { return lds_u8(SM + kFx2EX + i); }
    __device__ __forceinline__ uint32_t roots(const uint32_t i) const { return root_tbl[i]; }
};

// fx2_fix_block for R = 6 with the closed form in front
template <uint32_t SMB = 0>
__device__ __forceinline__ bool fx3_fix_block(const uint32_t lo, const uint32_t hi, const uint32_t yb, const uint32_t* __restrict__ root_tbl, const uint32_t FMA) {
    constexpr uint32_t K = 20;
    uint32_t S[6];
#pragma unroll
    for (uint32_t j = 0; j < 6u; ++j) S[j] = ((j < 3u ? lo : hi) >> (8u * (j % 3u))) & 0xFFu;
    Solve3 r = fx2_solve<6>(Fx3Lds<SMB>{FMA, root_tbl}, S);
    bool ok = true;
    if (__builtin_amdgcn_ballot_w64(r.np == 0u) != 0) {                             // (wave-uniform) some lane's block is not a plain 2 or 3 errors
        if (r.np == 0u) {
            Fix fx; fx.np = 0;
            ok = fx2_correct<6, SMB, true>(S, fx, root_tbl, FMA) == 0u;
            if (ok) { r.np = fx.np;
#pragma unroll
                for (int q = 0; q < 3; ++q) { r.pos[q] = fx.pos[q]; r.mag[q] = fx.mag[q]; } }
        }
    }
    if (!ok) return false;
    // the patches side by side, as fx2_fix_block's: a slot that patches nothing works on the dummy bytes
    uint32_t ad[3], yv[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) { ad[q] = ((uint32_t)q < r.np && r.pos[q] < K) ? yb + 9u * r.pos[q] : SMB + kFx2Dummy + 4u * (uint32_t)q; yv[q] = lds_u8(ad[q]); }
#pragma unroll
    for (int q = 0; q < 3; ++q) yv[q] = lds_u8(FMA + (54u + r.mag[q]) * 27u + min(yv[q], 26u));   // y - m = y + 2 m  (dummy bytes may hold anything)
#pragma unroll
    for (int q = 0; q < 3; ++q) *T3_LDS(uint8_t, ad[q]) = (uint8_t)yv[q];
    return true;
}

// fx2_queue_entry for R = 6
template <uint32_t SMB = 0>
__device__ __forceinline__ void fx3_queue_entry(const uint32_t* __restrict__ roots, const uint32_t fma_off, uint32_t* fail, const uint32_t e, const uint32_t q_off, const uint32_t qcap, const uint32_t y_off) {
    const u32x2 sy = *T3_LDS(const u32x2, q_off + 8u * e);
    const uint32_t tag = *T3_LDS(const uint16_t, q_off + 8u * qcap + 2u * e);
    if (!fx3_fix_block<SMB>(sy.x, sy.y, y_off + tag, roots, fma_off)) atomicAdd(fail, 1u);
}

}  // namespace
}  // namespace t3
