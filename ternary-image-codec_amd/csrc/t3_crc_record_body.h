// t3_crc_record_body.h — what the table CRC kernels and the frame record kernels share: crc_chunks_kernel / frame_record_kernel
// (t3_decode.hip, one stream) and crc_chunks_frames_kernel / frame_records_kernel (t3_crc_frames.hip, N equal streams).  The device
// helpers of the table kernels (their common body is t3_crc_chunks_body.inc) and the record kernels' load-and-fold.  Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/t3hip.h"
#include "t3_crc.h"

namespace t3 {

// ---- CRC-32 (poly 0xEDB88320, io_t3p_t3v.cpp:18-33) over the payload, in parallel -----------------------------
// Register update is GF(2)-linear: R(x, A||B) = Z_{|B|} R(x, A) ^ R(0, B).  Each lane takes a chunk, computes
// R(0, chunk), moves it to the end of the stream with the "append zero bytes" operators and XORs it in.
__device__ __forceinline__ uint32_t gf2_apply(const uint32_t* col, uint32_t x) {
    uint32_t y = 0;
#pragma unroll
    for (int i = 0; i < 32; ++i) y ^= (x >> i & 1u) ? col[i] : 0u;
    return y;
}

// append `n` zero bytes to register x: one operator per set bit of n
__device__ __forceinline__ uint32_t crc_shift(const uint32_t* zpow, uint32_t x, uint64_t n) {
    for (int j = 0; n; ++j, n >>= 1) if (n & 1u) x = gf2_apply(zpow + 32 * j, x);
    return x;
}

// One lane = one chunk, taken as two halves in lockstep (two independent register chains), a 32-bit word per step and
// chain by slicing-by-4: four independent table reads instead of four dependent ones.  The four 256-entry tables sit in
// LDS in four copies each (copy = lane & 3).  Measured alternatives (8K frame, 187 MB): one dependent byte-table chain per
// lane 147 us; this kernel 127 us; byte table in 32 per-bank copies with four chains 175 us; a coalesced row sweep with
// advance tables 193 us (profiles/r01/notes.md).
__device__ __forceinline__ uint32_t crc_word(const uint32_t* tb, uint32_t cp, uint32_t r, uint32_t w) {
    r ^= w;
    return tb[((3u * 256u + (r & 0xFFu)) << 2) + cp] ^ tb[((2u * 256u + ((r >> 8) & 0xFFu)) << 2) + cp] ^
           tb[((1u * 256u + ((r >> 16) & 0xFFu)) << 2) + cp] ^ tb[((r >> 24) << 2) + cp];
}
// One wave, one load-and-fold.  The CRC kernel left the stream's remainder without its leading 0xFFFFFFFF as the XOR of its (xor, sum)
// pairs -- n_partials of them side by side in `partials`, or one in acc[0..1] -- the rest behind the last whole round included.
// lead = the leading 0xFFFFFFFF carried through n_bytes zero bytes (host: square-and-multiply on the operator).  Every load is issued
// before the first wait, at clamped addresses: one dword per lane and step (64 is even, so even lanes read only xor words and odd lanes
// only sum words) and the lane's header byte; shuffles fold them.  (The kernel used to fold the rest itself, bit-serially: the
// compiler made the bit loop a table in global memory, 32 dependent loads per lane, and the kernel took 14 us behind the decoder.)
__device__ __forceinline__ void frame_record_body(const uint32_t* acc, uint32_t lead, const uint8_t* words, uint64_t n_words, uint64_t frame_idx,
                                                  uint32_t profile, uint32_t mode, t3_frame_record* rec, const uint32_t* partials, uint32_t n_partials) {
    const uint32_t lane = threadIdx.x;
    constexpr uint32_t kSteps = 2u * kRecordPartialWgs / 64u;
    const uint32_t* src = n_partials ? partials : acc;
    const uint32_t n_dw = n_partials ? 2u * n_partials : 2u;                             // <= 64 kSteps (plan_crc)
    const uint32_t n_hdr = n_words >= 6u ? 54u : 9u * (uint32_t)n_words;
    uint32_t v[kSteps];
#pragma unroll
    for (uint32_t k = 0; k < kSteps; ++k) v[k] = src[min(lane + 64u * k, n_dw - 1u)];
    const uint32_t h = n_hdr ? words[min(lane, n_hdr - 1u)] : 0u;
    uint32_t ax = 0, as = 0;
#pragma unroll
    for (uint32_t k = 0; k < kSteps; ++k) {
        const uint32_t e = lane + 64u * k < n_dw ? v[k] : 0u;
        if (lane & 1u) as += e; else ax ^= e;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { ax ^= __shfl_xor(ax, o); as += __shfl_xor(as, o); }
    if (lane == 0) {
        rec->frame_idx = frame_idx; rec->n_words = n_words; rec->byte_offset = 0;
        rec->crc32 = (lead ^ ax) ^ 0xFFFFFFFFu; rec->sym_sum = as;                           // final inversion
        rec->profile = (uint8_t)profile; rec->mode = (uint8_t)mode;
        for (int i = 0; i < 8; ++i) rec->pad_[i] = 0;
    }
    if (lane < 54) rec->header_syms[lane] = lane < n_hdr ? h : 0;
}

}  // namespace t3
