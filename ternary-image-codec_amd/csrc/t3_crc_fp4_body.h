// t3_crc_fp4_body.h — the device helpers of the matrix-core CRC-32 kernels crc_fp4_kernel (t3_crc_fp4.hip, one stream; it has the
// account of the method) and crc_fp4_frames_kernel (t3_crc_frames.hip, N equal streams); their common body is t3_crc_fp4_body.inc.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "t3_crc.h"

#ifndef T3_CRC_DEPTH
#define T3_CRC_DEPTH 4
#endif
#ifndef T3_CRC_NT
#define T3_CRC_NT 0
#endif

namespace t3 {

typedef int v8i_ __attribute__((ext_vector_type(8)));
typedef float v16f_ __attribute__((ext_vector_type(16)));

namespace {
typedef float v2f_ __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint4 ld16(const uint8_t* q) {
#if T3_CRC_NT
    typedef uint32_t u4_ __attribute__((ext_vector_type(4)));
    const u4_ v = __builtin_nontemporal_load((const u4_*)q); return make_uint4(v[0], v[1], v[2], v[3]);
#else
    return *(const uint4*)q;
#endif
}
// Wave reductions without LDS traffic: four DPP steps inside a row of 16 lanes (quad_perm 1032, quad_perm 2301, row_half_mirror,
// row_mirror), then the four rows by readlane.  The result is wave-uniform.  (__shfl_xor is one ds_bpermute_b32 per step, each waited
// for before the next: six LDS round trips where this is ~10 register instructions.)
template <int kCtrl> __device__ __forceinline__ uint32_t dpp_(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, kCtrl, 0xF, 0xF, true); }
__device__ __forceinline__ uint32_t rows_(uint32_t v, bool add) {
    const uint32_t r0 = __builtin_amdgcn_readlane((int)v, 0), r1 = __builtin_amdgcn_readlane((int)v, 16), r2 = __builtin_amdgcn_readlane((int)v, 32), r3 = __builtin_amdgcn_readlane((int)v, 48);
    return add ? r0 + r1 + r2 + r3 : r0 ^ r1 ^ r2 ^ r3;
}
__device__ __forceinline__ uint32_t wave_xor(uint32_t v) {
    v ^= dpp_<0xB1>(v); v ^= dpp_<0x4E>(v); v ^= dpp_<0x141>(v); v ^= dpp_<0x140>(v);
    return rows_(v, false);
}
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
    v += dpp_<0xB1>(v); v += dpp_<0x4E>(v); v += dpp_<0x141>(v); v += dpp_<0x140>(v);
    return rows_(v, true);
}
// a GF(2) operator on the wave-uniform register x: lane b < 32 holds the operator's column b
__device__ __forceinline__ uint32_t wave_apply_col(uint32_t col, uint32_t x, uint32_t lane) {
    return wave_xor((lane < 32u && ((x >> lane) & 1u)) ? col : 0u);
}
__device__ __forceinline__ uint32_t wave_apply4(const uint32_t* __restrict__ op, uint32_t x, uint32_t lane) {
    return wave_apply_col(lane < 32u ? op[lane] : 0u, x, lane);
}
__device__ __forceinline__ v16f_ mfma4(const uint32_t (&A)[4], const uint32_t b0, const uint32_t b1, const uint32_t b2, const uint32_t b3, const v16f_ acc) {
    const v8i_ a = {(int)A[0], (int)A[1], (int)A[2], (int)A[3], 0, 0, 0, 0}, b = {(int)b0, (int)b1, (int)b2, (int)b3, 0, 0, 0, 0};
    return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, acc, 4, 4, 0, 0x7F7F7F7F, 0, 0x7F7F7F7F);     // cbsz = blgp = 4: FP4; scales 2^0
}
// the 16 remainder bits a lane holds (parities of its accumulators) as FP4 0.5 in K slots 8 g + q of its half: accumulator 4 g + q ->
// dword g, nibble q
__device__ __forceinline__ void parity_nibbles(const v16f_& acc, uint32_t (&f)[4]) {
    const v2f_ m01 = {8388608.0f, 524288.0f}, m23 = {32768.0f, 2048.0f};           // 2^23, 2^19, 2^15, 2^11
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const v2f_ lo = v2f_{acc[4 * g], acc[4 * g + 1]} + m01, hi = v2f_{acc[4 * g + 2], acc[4 * g + 3]} + m23;
        f[g] = (__float_as_uint(lo[0]) & 0x1u) | (__float_as_uint(lo[1]) & 0x10u) | (__float_as_uint(hi[0]) & 0x100u) | (__float_as_uint(hi[1]) & 0x1000u);
    }
}
// one round's data: the lane's 32 bytes (bytes 4 s .. 4 s + 3 in w[s]) through the eight data slices, on top of acc
__device__ __forceinline__ v16f_ mfma_round(const uint32_t (&A)[9][4], const uint32_t (&w)[8], v16f_ acc) {
#pragma unroll
    for (int s = 0; s < 8; ++s) acc = mfma4(A[s], w[s] & 0x11111111u, w[s] & 0x22222222u, w[s] & 0x44444444u, (w[s] >> 1) & 0x44444444u, acc);
    return acc;
}
}  // namespace

}  // namespace t3
