// t3_repair.h — argument blocks and kernel declarations of the FIXED stream repair (t3_repair.hip, launched by t3_api_repair.cpp).  The
// fused kernels' arguments are the decode planner's repair form (t3_dec_plan.hpp), bound by bind_fused (t3_ctx.hpp).
#pragma once
#include <stdint.h>

#include "t3_decode.h"

namespace t3 {

// What either kernel does beside the blocks: the bytes behind the framed body up to the frame's last word become 0 (workgroup 0), and the
// launch adds its counts to verdict[1..3] (zeroed in front of it; verdict[0] is hdr_compare_kernel's).
struct RepairEdge {
    uint8_t* io;                  // the frame: header, framed body, tail
    uint32_t* verdict;            // [1] uncorrectable blocks, [2] blocks changed, [3] bytes changed; the erasure kernels also [4], [5]
    uint32_t write;               // T3_REPAIR_WRITE; 0: a dry run, same counts, no store
    uint32_t tail_len;            // < 9
    uint32_t tail_skip;           // the tail byte that is a beacon slot, else 0xFFFFFFFF
    uint64_t tail_off;            // from io
};
// repair_fixed_kernel<R>: the fused decoder's argument block as it is (a.in = the frame, a.out / a.n_units unused) and the edge
struct RepairFxArgs { DecFx2Args a; RepairEdge e; };
// repair_generic_kernel: the generic decoder's index map (d.fixed = 1, d.use unused) and the beacon slots: n_bcn of them, slot j at framed
// body byte bcn_first + j * bcn_step, each becomes bcn_sym
struct RepairGenArgs { DecArgs d; RepairEdge e; uint64_t n_bcn, bcn_first, bcn_step; uint32_t bcn_sym; };
// repair_frames_kernel<R> (t3_repair_frames.hip): a batch of equal frames in one launch.  r: the arguments of frame 0 as they are; frame f
// lies f * stride bytes (even) behind it and owns verdict words 4 f .. 4 f + 3 (r.e.verdict: those of frame 0).  Global tile t names
// frame t / r.a.n_tiles and tile t % r.a.n_tiles of it.
struct RepairFramesArgs {
    RepairFxArgs r;
    uint64_t stride;
    uint32_t n_frames, n_total;                // n_total = n_frames * r.a.n_tiles < 2^31
    DevDiv div_tiles;                          // by r.a.n_tiles
};
// erasure_frames_kernel<R> (t3_repair_era_frames.hip): the same block; frame f owns verdict words 6 f .. 6 f + 5 (the verdict stride is
// the kernel's own constant)
using EraFramesArgs = RepairFramesArgs;

#if defined(__HIPCC__)
template <int R> __global__ void repair_fixed_kernel(const RepairFxArgs ra);
__global__ void repair_generic_kernel(const RepairGenArgs ra);
template <int R> __global__ void repair_frames_kernel(const RepairFramesArgs fa);
__global__ void hdr_compare_frames_kernel(const uint8_t* in, uint64_t stride, HdrExpect expect, uint32_t n, uint32_t nw, uint32_t* verdict);   // one workgroup per frame -> verdict[nw f]
// t3_repair_era.hip: bytes above 26 taken as erasures.  The argument blocks of the plain kernels; verdict words [1..5]
template <int R> __global__ void erasure_fixed_kernel(const RepairFxArgs ra);
__global__ void erasure_generic_kernel(const RepairGenArgs ra);
__global__ void rs_erasure_blocks_kernel(uint8_t* code, uint64_t n_blocks, int k, const RsTables* tab, uint8_t* data, uint8_t* ok);
// t3_repair_era_frames.hip: the batch form, verdict words 6 f .. 6 f + 5
template <int R> __global__ void erasure_frames_kernel(const EraFramesArgs fa);
#endif

}  // namespace t3
