// t3_repair_tile.h — what the fused repair kernels do around the block stages (t3_repair_blocks.h), shared by the single-frame kernel
// (t3_repair.hip) and the batch kernel (t3_repair_frames.hip): the frame's tail bytes, and the bytes-above-26 test kept per block.
#pragma once
#include "t3_decode_fx2.h"
#include "t3_repair.h"

namespace t3 {
namespace {
// the bytes behind the framed body of the frame at `io`: one thread each
__device__ __forceinline__ uint32_t rp_tail(const RepairEdge& e, uint8_t* const io, const uint32_t tid) {
    if (tid >= e.tail_len || tid == e.tail_skip) return 0u;             // (a beacon slot among them is the beacon loop's)
    uint8_t* const p = io + e.tail_off + tid;
    if (*p == 0) return 0u;
    if (e.write) *p = 0;
    return 1u;
}
// any of the lane's 13 symbols (positions 13 h .. 13 h + 12 of its block, fx2_set's W) above 26?
__device__ __forceinline__ bool rp_high13(const uint32_t (&Lw)[4], const uint32_t h) {
    uint32_t W[4];
#pragma unroll
    for (int i = 0; i < 3; ++i) W[i] = __builtin_amdgcn_alignbyte(Lw[i + 1], Lw[i], 3u * h);
    W[3] = Lw[3] >> (24u * h);
    uint32_t hi = (W[3] | (W[3] + 0x65u)) & 0x80u;
#pragma unroll
    for (int i = 0; i < 3; ++i) hi |= (W[i] | (W[i] + 0x65656565u)) & 0x80808080u;
    return hi != 0u;
}
}  // namespace
}  // namespace t3
