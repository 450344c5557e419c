// t3_crc.h — CRC-32 and frame index record: argument blocks and kernel declarations (host side: t3_api_record.cpp).
#pragma once
#include <stdint.h>

#include "../../include/t3hip.h"

namespace t3 {

constexpr int kCrcPows = 40;                     // "append 2^j zero bytes" operators, j < kCrcPows
struct CrcArgs {
    const uint8_t* data; uint64_t n_bytes; uint32_t chunk_bytes; uint32_t n_chunks;
    uint32_t* chunk_crc; uint32_t* sym_sum;      // device accumulators, zeroed by the launcher
    const uint32_t* zpow;                        // [kCrcPows][32] operator columns (device)
};

// CRC-32 on the matrix cores (t3_crc_fp4.hip): whole 2 KiB rounds of a 16-byte aligned stream and the rest behind them (tail_len)
struct CrcMArgs {
    const uint8_t* data; uint64_t n_bytes;       // whole stream (distance to its end)
    uint32_t n_rounds, rounds_per_wave;          // 2 KiB rounds in total / per wave
    uint32_t stride_waves;                       // 0 = a wave owns rounds_per_wave consecutive rounds; W > 0 = wave g owns rounds g, g + W, g + 2 W ..
    const uint32_t* afb;                         // ... and its feedback slice [64][4] ("append 2048 W zero bytes") comes from here
    const uint32_t* afrag;                       // [14][64][4] FP4 slices: 8 data slices, the feedback slice, five "append 64 * 2^b bytes" slices, in MFMA lane order
    const uint32_t* zpow;                        // blocked form only: its epilogue walks the distance bit by bit
    // strided form: wave g's last round is n_rounds - 1 - hi with hi = (last_mod - g) mod W, so its remainder stands tail_len + 2048 hi
    // bytes before the stream's end: one column per lane of dist_lo[tail_len] and of dist_hi[hi], loaded at kernel entry
    const uint32_t* dist_lo;                     // [2048][32] "append n bytes"
    const uint32_t* dist_hi;                     // [W0 + 1][32] "append 2048 n bytes"
    uint32_t last_mod;                           // (n_rounds - 1) mod W
    uint32_t* chunk_crc; uint32_t* sym_sum;
    uint32_t* partials;                         // != null: workgroup g stores its (xor, sum) at [2 g], [2 g + 1] instead of adding to the two accumulators (no zeroing pass, no atomics)
    uint32_t tail_len;                           // the n_bytes - 2048 n_rounds < 2048 bytes behind the last round; != 0: workgroup 0 takes them, the rounds start at workgroup 1
};
constexpr uint32_t kRecordPartialWgs = 1024;     // most (xor, sum) partials frame_record_kernel folds

// N equal streams in one launch (t3_crc_frames.hip; blockIdx.y = frame f).  m / t describe frame 0: its stream at data, its
// accumulator pair at chunk_crc / sym_sum, its partials (FP4, or null) -- frame f's are f * stride bytes (stream) and f * slot_bytes
// bytes (accumulators, partials) further on.  Everything else is the same for every frame.
constexpr uint32_t kSlotPartialsOff = 64;        // a slot: the accumulator pair at its start, the partials from this byte on
struct CrcFramesArgs { CrcMArgs m; uint64_t stride; uint32_t slot_bytes, n_frames; };
struct CrcChunksFramesArgs { CrcArgs t; uint64_t stride; uint32_t slot_bytes, n_frames; };
// frame_records_kernel: one wave per frame folds slot f (n_partials pairs from kSlotPartialsOff on, or the pair at its start) and
// writes recs[f] with frame_idx = first_idx + f * idx_step
struct RecordsArgs {
    const uint8_t* scratch; uint32_t slot_bytes, n_partials;
    const uint8_t* words; uint64_t stride, n_words;
    uint64_t first_idx, idx_step;
    uint32_t lead, profile, mode;
    t3_frame_record* recs;
};

#if defined(__HIPCC__)
__global__ void crc_fp4_frames_kernel(const CrcFramesArgs a);
__global__ void crc_chunks_frames_kernel(const CrcChunksFramesArgs a);
__global__ void frame_records_kernel(const RecordsArgs a);
__global__ void crc_chunks_kernel(const CrcArgs a);
__global__ void crc_fp4_kernel(const CrcMArgs a);
__global__ void frame_record_kernel(const uint32_t* acc, uint32_t lead, const uint8_t* words, uint64_t n_words, uint64_t frame_idx, uint32_t profile, uint32_t mode, void* rec, const uint32_t* partials, uint32_t n_partials);
#endif

}  // namespace t3
