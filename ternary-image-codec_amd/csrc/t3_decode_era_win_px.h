// t3_decode_era_win_px.h — the pixel stage of the erasure decoder's window kernels: a lane's 12 pixels of a tile, each stored at its WINDOW
// position or nowhere.  One text for decode_era_window_px (t3_decode_era_window.hip; out_off = 0) and its batch form
// decode_era_frames_window_px (t3_decode_era_frames_window.hip; out_off = the frame's f * out_stride).
#pragma once
#include <stdint.h>

#include "t3_decode.h"
#include "t3_decode_px.h"

namespace t3 {

namespace {
// D5 for lane slot j of a tile, into the window: units [12 j, 12 j + 12) of the tile whose first unit is stream pixel p_tile; n_here: the
// tile's units that exist.  out_off: the window's first byte behind wa.a.out (a multiple of 16: the 4-byte test of the fast path holds
// with it as without).  RGB: fx2_pixels12<true>'s conversion, step for step (t3_decode_px.h)
template <bool RGB>
__device__ __forceinline__ void era_win_pixels12(const DecEraWinArgs& wa, const uint32_t j, const uint32_t y_off, const uint32_t p_tile, const uint32_t n_here, const uint64_t out_off) {
    constexpr uint32_t B = RGB ? 3u : 6u;
    const DecFx2Args& a = wa.a;
    const uint32_t u0 = 12u * j;
    if (u0 >= n_here) return;
    const uint32_t p0 = p_tile + u0;
    uint32_t row = div_any(p0, wa.div_fw), col = p0 - row * wa.fw;
    if (row >= wa.rows_end) return;                                                 // (rows only grow along the group)
    const uint32_t x1 = wa.x0 + wa.w;                                                // (<= fw: the planner)
    const bool one_row = col + 12u <= wa.fw;                                         // the group lies in one frame row (p0 < 2^31: no wrap)
    if (one_row && (row < wa.y0 || col + 12u <= wa.x0 || col >= x1)) return;         // ... and above the window or beside its columns
    uint32_t D[13];
#pragma unroll
    for (int i = 0; i < 13; ++i) D[i] = *T3_LDS(const uint32_t, y_off + 52u * j + 4u * i);
    uint32_t o[18];
    px12_from_syms(D, o);
    uint32_t q[RGB ? 9 : 18];                                                        // the group's output bytes, in order
    if constexpr (RGB) {
#pragma unroll
        for (uint32_t i = 0; i < 9; ++i) q[i] = 0u;
#pragma unroll
        for (uint32_t p = 0; p < 12; ++p) {
            auto comp = [&](uint32_t k) -> uint32_t { return (o[k >> 1] >> (16u * (k & 1u))) & 0xFFFFu; };
            const uint32_t Yq = min(comp(3u * p), 242u);
            const int cbq = max(-40, min(40, (int)(int16_t)comp(3u * p + 1u))), crq = max(-40, min(40, (int)(int16_t)comp(3u * p + 2u)));
            const float y = (float)lds_u8(a.dq_off + Yq);
            const float cb = __fsub_rn((float)lds_u8(a.dq_off + 244u + (uint32_t)(cbq + 40)), 128.0f), cr = __fsub_rn((float)lds_u8(a.dq_off + 244u + (uint32_t)(crq + 40)), 128.0f);
            const float r = __fadd_rn(y, __fmul_rn(1.402f, cr));
            const float g = __fsub_rn(__fsub_rn(y, __fmul_rn(0.344136f, cb)), __fmul_rn(0.714136f, cr));
            const float b = __fadd_rn(y, __fmul_rn(1.772f, cb));
            const uint32_t c3[3] = {min((uint32_t)__fadd_rn(r, 0.5f), 255u), min((uint32_t)__fadd_rn(g, 0.5f), 255u), min((uint32_t)__fadd_rn(b, 0.5f), 255u)};
#pragma unroll
            for (uint32_t k = 0; k < 3; ++k) { const uint32_t bi = 3u * p + k; q[bi >> 2] |= c3[k] << (8u * (bi & 3u)); }
        }
    } else {
#pragma unroll
        for (uint32_t i = 0; i < 18; ++i) q[i] = o[i];
    }
    uint8_t* const out = (uint8_t*)a.out + out_off;
    if (one_row && u0 + 12u <= n_here && col >= wa.x0 && col + 12u <= x1) {          // (row >= y0: the test above) all 12 in one window row
        const uint64_t off = ((uint64_t)(row - wa.y0) * wa.w + (col - wa.x0)) * B;
        if ((off & 3u) == 0u) {                                                      // a.out + out_off is 4-byte aligned
            uint32_t* const g = (uint32_t*)(out + off);
#pragma unroll
            for (uint32_t i = 0; i < (RGB ? 9u : 18u); ++i) g[i] = q[i];
            return;
        }
    }
#pragma unroll
    for (uint32_t i = 0; i < 12; ++i) {
        if (u0 + i < n_here && row >= wa.y0 && row < wa.rows_end && col >= wa.x0 && col < x1) {
            uint8_t* const g = out + ((uint64_t)(row - wa.y0) * wa.w + (col - wa.x0)) * B;
            if constexpr (RGB) {
#pragma unroll
                for (uint32_t k = 0; k < 3; ++k) { const uint32_t bi = 3u * i + k; g[k] = (uint8_t)(q[bi >> 2] >> (8u * (bi & 3u))); }
            } else {
#pragma unroll
                for (uint32_t k = 0; k < 3; ++k) { const uint32_t hi = 3u * i + k; *(uint16_t*)(g + 2u * k) = (uint16_t)(q[hi >> 1] >> (16u * (hi & 1u))); }
            }
        }
        if (++col == wa.fw) { col = 0u; ++row; }
    }
}
}  // namespace

}  // namespace t3
