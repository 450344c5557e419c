// t3_crc_fp4.hip — CRC-32 of the coded payload on the matrix cores (crc32_acc, src/io_t3p_t3v.cpp:20-36; the T3V frame index and the
// payload CRC of the containers), on the block-scaled FP4 instruction of gfx950.
//
// The CRC register update is GF(2)-linear, so the remainder of a 64-byte chunk is a 32 x 512 bit matrix (A, host-built in slices) times
// the chunk's bits.  Column n of the B operand = chunk n of the wave's current 2 KiB: a wave reads 2 KiB per round perfectly coalesced
// (lane (n, h) takes bytes 64 n + 32 h .. + 32).  The column's running remainder re-enters as more K inputs through the feedback slice,
// an "append zero bytes" matrix over the distance to the column's next chunk.  After the last round a column's remainder moves to the end
// of the stream: 64 (31 - n) bytes per column (five masked steps through the "append 64 * 2^b bytes" slices), then, XOR-reduced over
// the columns, the common distance with one operator column per lane.  v_mfma_scale_f32_32x32x64_f8f6f4
// with FP4 (e2m1) operands runs 64 K values per instruction in the cycles the i8 instruction needs for 32: a 2 KiB round is 8 data
// instructions + 1 feedback instead of 16 + 1.  Block scales 2^0 (e8m0 127); every product is 0 or exactly 1, a dot product is at most
// 512 + 16, exact in f32; the remainder bit is the parity of its integer value.
// Round 3: no table, no LDS in the loop.  An input dword becomes its four B dwords with five vector instructions: w & 0x11111111,
// w & 0x22222222, w & 0x44444444 and (w >> 1) & 0x44444444 -- a bit stays where it is inside its nibble and therefore reads as FP4 0.5, 1.0
// or 2.0; the matrix slice holds the reciprocal weight (2.0, 1.0, 0.5) in that K slot, so the product is 1.  (Round 2 read a 256-entry
// byte -> eight-nibble table, 32 bank copies: two vector instructions + one LDS read per BYTE, and the compiler's schedule put the LDS
// latency of every step in series with its matrix instruction: ~1,100 cycles per round and SIMD.)  Which K slot carries which bit is free
// (the hardware pairs position p of lane half kh in A with the same position in B): the host builds the slices in the order the
// kernel feeds bits (t3_api_record.cpp, crc_init).
// Parity without a conversion: x = acc + 2^(23 - s) has the integer's bit 0 at mantissa bit s (the sum is exact: acc < 2^11); with
// s = 0, 4, 8, 12 for the four accumulators of a group the bits land in nibbles 0..3 of one dword at nibble bit 0 (FP4 0.5, weight 2.0 in
// the feedback slice): a packed add per two accumulators and one v_and_or per accumulator.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/t3hip.h"
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

__global__ __launch_bounds__(256) void crc_fp4_kernel(const CrcMArgs a) {
    __shared__ uint32_t red[2 * 16];
    const uint32_t lane = threadIdx.x & 63u, n = lane & 31u, kh = lane >> 5, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // The rest behind the last whole round (tail_len < 2048 bytes) belongs to wave 0 of workgroup 0, dispatched first and done long before
    // the streaming waves; the rounds start at workgroup 1.  (Composed at the end of the kernel, the rest was on its critical path.)
    const uint32_t tail_wg = a.tail_len ? 1u : 0u;
    const bool in_tail_wg = blockIdx.x < tail_wg;
    const uint32_t wave_g = (blockIdx.x - tail_wg) * (blockDim.x >> 6) + wave;
    // Which rounds a wave owns.  Strided (stride_waves = W > 0): wave g takes rounds g, g + W, g + 2 W ... -- at any moment the chip reads one
    // moving window of W x kDepth x 2 KiB, the way a streaming copy does; a wave on rounds_per_wave consecutive rounds of its own makes
    // the chip read at 2048 places 90 KB apart, 2 KiB at a time (3.4 TB/s against the 4.5+ a read-only stream reaches).  A column's next
    // chunk is then 2048 W bytes further on: the feedback slice is the host-built "append 2048 W zero bytes" operator (a.afb).
    const uint32_t W = a.stride_waves;
    uint64_t r0, r1, step;                                                          // rounds r0, r0 + step, ... < r1
    if (in_tail_wg) { r0 = r1 = 0; step = 1; }
    else if (W) { r0 = wave_g; r1 = a.n_rounds; step = W; }
    else { r0 = min((uint64_t)wave_g * a.rounds_per_wave, (uint64_t)a.n_rounds); r1 = min(r0 + a.rounds_per_wave, (uint64_t)a.n_rounds); step = 1; }   // a wave past the end runs zero rounds
    const uint64_t pstep = 2048u * step;
    const uint8_t* p = a.data + r0 * 2048u + 64u * n + 32u * kh;
    const v16f_ zero = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t f[4] = {0, 0, 0, 0}, sum = 0;
    // Rounds are latency-bound, not arithmetic-bound: with one round of loads in flight per wave a round took ~2,800 cycles (the memory
    // latency under load) against ~600 of arithmetic; kDepth rounds are kept in flight (8 registers each).
    constexpr uint32_t kDepth = T3_CRC_DEPTH;
    uint4 Q[kDepth][2];
    // A streaming wave's first memory instructions are its first kDepth rounds of payload: all workgroups start together, and whatever
    // stands in front of these loads is a stretch in which the chip reads no payload at all.  The operator slices follow them, and no
    // barrier stands between kernel entry and the round loop.
#pragma unroll
    for (uint32_t d = 0; d < kDepth; ++d) { Q[d][0] = make_uint4(0, 0, 0, 0); Q[d][1] = Q[d][0]; if (r0 + d * step < r1) { Q[d][0] = ld16(p + pstep * d); Q[d][1] = ld16(p + pstep * d + 16); } }
    __builtin_amdgcn_sched_barrier(0);
    uint32_t A[9][4];
#pragma unroll
    for (int s = 0; s < 9; ++s) {
        const uint4 q = (s == 8 && W) ? *(const uint4*)(a.afb + (size_t)lane * 4u) : *(const uint4*)(a.afrag + ((size_t)s * 64u + lane) * 4u);
        A[s][0] = q.x; A[s][1] = q.y; A[s][2] = q.z; A[s][3] = q.w;
    }
    // Strided form: the wave's last round is known here, and with it the distance from the end of that round to the stream's end,
    // tail_len + 2048 hi bytes with hi = (last_mod - g) mod W < W.  One column per lane of the two table operators (t3_crc.h); the
    // workgroup that takes the rest, and a wave without rounds, keep distance 0 (entry 0 = identity).
    uint32_t dcol_lo = 0, dcol_hi = 0;
    if (W) {
        const bool moves = !in_tail_wg && wave_g < W && r0 < r1;
        const uint32_t hi = moves ? (a.last_mod >= wave_g ? a.last_mod - wave_g : a.last_mod + W - wave_g) : 0u;
        dcol_lo = a.dist_lo[(moves ? a.tail_len : 0u) * 32u + n];
        dcol_hi = a.dist_hi[hi * 32u + n];
    }
    for (uint64_t r = r0; r < r1; r += kDepth * step, p += pstep * kDepth) {
#pragma unroll
        for (uint32_t d = 0; d < kDepth; ++d) {
            if (r + d * step >= r1) break;
            const uint32_t w[8] = {Q[d][0].x, Q[d][0].y, Q[d][0].z, Q[d][0].w, Q[d][1].x, Q[d][1].y, Q[d][1].z, Q[d][1].w};
            if (r + (d + kDepth) * step < r1) { Q[d][0] = ld16(p + pstep * (d + kDepth)); Q[d][1] = ld16(p + pstep * (d + kDepth) + 16); }   // kDepth rounds ahead, in flight from here on
#pragma unroll
            for (int i = 0; i < 8; ++i) sum = __builtin_amdgcn_sad_u8(w[i], 0u, sum);
            parity_nibbles(mfma_round(A, w, mfma4(A[8], f[0], f[1], f[2], f[3], zero)), f);   // running remainder one round step further on, plus this round
        }
    }
    if (in_tail_wg && wave == 0) {
        // The rest as one round of its own that ends at the stream's end: bytes in front of the rest read as zero (they do not move a
        // zero remainder), so after the column alignment below its remainder is in place and needs no shift.  Lane (n, kh) holds round
        // bytes 64 n + 32 kh .. + 31, i.e. rest bytes from lo on; lanes with leading zeros only load nothing.  Byte loads at clamped
        // addresses: all in flight together, none past the stream's end.
        const uint8_t* t = a.data + ((uint64_t)a.n_rounds << 11);
        const int32_t lo = (int32_t)(64u * n + 32u * kh + a.tail_len) - 2048;
        uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (lo > -32) {
            uint32_t b[32];
#pragma unroll
            for (int32_t i = 0; i < 32; ++i) b[i] = t[max(lo + i, 0)];
#pragma unroll
            for (int32_t i = 0; i < 32; ++i) w[i >> 2] |= (lo + i >= 0 ? b[i] : 0u) << (8 * (i & 3));
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) sum = __builtin_amdgcn_sad_u8(w[i], 0u, sum);
        parity_nibbles(mfma_round(A, w, zero), f);
    }
    // Column n's remainder stands at the end of its last chunk, 64 (31 - n) bytes before the end of the wave's region: five masked steps
    // through the "append 64 * 2^b zero bytes" matrices (slices 9..13) bring every column to the region end
#pragma unroll
    for (int b = 0; b < 5; ++b) {
        const uint4 q = *(const uint4*)(a.afrag + ((size_t)(9 + b) * 64u + lane) * 4u);
        const uint32_t Ab[4] = {q.x, q.y, q.z, q.w};
        uint32_t m[4]; parity_nibbles(mfma4(Ab, f[0], f[1], f[2], f[3], zero), m);
        if (((31u - n) >> b) & 1u) { f[0] = m[0]; f[1] = m[1]; f[2] = m[2]; f[3] = m[3]; }
    }
    // This lane's 16 bits -> register bits (accumulator e = 4 g + q of half kh = row (e & 3) + 8 (e >> 2) + 4 kh), then XOR over the
    // columns: the two halves hold disjoint register bits, so one reduction over the whole wave does both
    uint32_t part = 0;
#pragma unroll
    for (uint32_t e = 0; e < 16; ++e) part |= ((f[e >> 2] >> (4u * (e & 3u))) & 1u) << ((e & 3u) + 8u * (e >> 2) + 4u * kh);
    part = wave_xor(part);
    sum = wave_sum(sum);
    if (W) part = wave_apply_col(dcol_hi, wave_apply_col(dcol_lo, part, lane), lane);
    else {
        // blocked form (measurement knob): the distance bit by bit through the "append 2^j zero bytes" operators, staged here so that the
        // strided form pays nothing for them (W is the same for the whole grid: every thread of the workgroup gets here)
        __shared__ uint32_t zp[kCrcPows * 32];
        for (uint32_t e = threadIdx.x; e < (uint32_t)kCrcPows * 32u; e += blockDim.x) zp[e] = a.zpow[e];
        __syncthreads();
        uint64_t rest = in_tail_wg ? 0u : a.n_bytes - r1 * 2048u;
        for (int j = 0; rest; ++j, rest >>= 1) if (rest & 1u) part = wave_apply4(zp + 32 * j, part, lane);
    }
    if (lane == 0) { red[2 * wave] = part; red[2 * wave + 1] = sum; }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t x = 0, t = 0;
        for (uint32_t w = 0; w < (blockDim.x >> 6); ++w) { x ^= red[2 * w]; t += red[2 * w + 1]; }
        if (a.partials) { a.partials[2u * blockIdx.x] = x; a.partials[2u * blockIdx.x + 1u] = t; }
        else { if (x) atomicXor(a.chunk_crc, x); if (t) atomicAdd(a.sym_sum, t); }
    }
}

}  // namespace t3
