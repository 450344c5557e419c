// t3_crc_frames.hip — CRC-32 and frame index records of N equal streams in one launch each (t3hip_frame_records_dev,
// t3hip_crc32_frames[_dev]; host side: t3_api_record.cpp, plan_crc_frames).  A coded 854 x 480 frame is ~1,100 rounds of 2 KiB: on its
// own it gets 128 of the chip's 2,048 wave slots, and N launches of that size leave most of the part idle N times over.  Here
// blockIdx.y is the frame: frame f's stream starts f * stride bytes behind frame 0's, and its workgroups leave their results in
// slot f of the caller's scratch (the accumulator pair at the slot's start, the partials kSlotPartialsOff bytes in), exactly as the
// single-stream kernels leave theirs in the whole scratch.  All frames are equally long, so rounds, rest, W, the feedback slice and the
// distance tables are the single-stream ones: the bodies are shared (t3_crc_fp4_body.inc, t3_crc_chunks_body.inc, frame_record_body) and no
// host table is new.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/t3hip.h"
#include "t3_crc.h"
#include "t3_crc_fp4_body.h"
#include "t3_crc_record_body.h"

namespace t3 {

// frame blockIdx.y of a batch: its stream starts stride bytes, its slot slot_bytes bytes behind those of the frame before it (the bodies
// ask for a slot only where frame 0 has one: no null pointer is moved)
#define T3_CRC_STREAM(p) ((p) + (uint64_t)blockIdx.y * args.stride)
#define T3_CRC_SLOT(p) ((uint32_t*)((uint8_t*)(p) + (uint64_t)blockIdx.y * args.slot_bytes))

// grid (workgroups per frame, n_frames): crc_fp4_kernel's protocol per frame -- workgroup 0 the rest behind the last round, wave g the
// rounds g, g + W, ..., payload loads first
__global__ __launch_bounds__(256) void crc_fp4_frames_kernel(const CrcFramesArgs args) {
    const CrcMArgs& a = args.m;
#include "t3_crc_fp4_body.inc"
}

// grid (workgroups per frame, n_frames): the table kernel for frames the FP4 form does not take; adds into frame f's accumulator pair
__global__ __launch_bounds__(256) void crc_chunks_frames_kernel(const CrcChunksFramesArgs args) {
    const CrcArgs& a = args.t;
#include "t3_crc_chunks_body.inc"
}

#undef T3_CRC_STREAM
#undef T3_CRC_SLOT

// grid n_frames, one wave each: frame_record_kernel's load-and-fold on slot f and frame f's first 54 bytes; 96 bytes out per frame
__global__ __launch_bounds__(64) void frame_records_kernel(const RecordsArgs a) {
    const uint32_t f = blockIdx.x;
    const uint8_t* slot = a.scratch + (uint64_t)f * a.slot_bytes;
    frame_record_body((const uint32_t*)slot, a.lead, a.words + (uint64_t)f * a.stride, a.n_words, a.first_idx + (uint64_t)f * a.idx_step, a.profile, a.mode,
                      a.recs + f, (const uint32_t*)(slot + kSlotPartialsOff), a.n_partials);
}

}  // namespace t3
