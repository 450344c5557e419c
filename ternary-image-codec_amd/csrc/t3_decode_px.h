// t3_decode_px.h — decode_fixed_px_kernel, the pixel form of the fused FIXED decoder (stages and wave roles: t3_decode_fused.hip), and
// dec_frames_px, the same tile loop over a batch of equal frames in one launch (instantiated in t3_decode_frames.hip).  In front of them
// the pieces they share with decode_fixed_kernel: a lane's coded run, constants -> LDS, the pixel output stage.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/t3hip.h"
#include "t3_decode.h"
#include "t3_decode_fx.h"
#include "t3_decode_fx2.h"
#include "t3_decode_fx3.h"
#include "t3_decode_wg.h"

namespace t3 {

namespace {
// A lane's 16 coded bytes, in flight.  BCN (beacon stripped in the loads, OLD:952-957): the run starts at framed offset
// g0 + (beacons in front of it); if the next beacon falls inside the run (after c < 16 body bytes) the run is 17 framed bytes long and
// x carries the 17th byte and c; run_bytes() closes the gap when the run is used.
template <bool BCN> struct Run { u32x4 w; };
template <> struct Run<true> { u32x4 w; uint32_t w4, x; };              // five aligned dwords that hold the (up to) 17 framed bytes; x = start byte | c << 8
template <bool BCN>
__device__ __forceinline__ Run<BCN> load_run(const DecFx2Args& a, const uint8_t* body, const uint32_t g0) {
    Run<BCN> r;
    if constexpr (!BCN) r.w = load16(body + g0);          // 2-byte aligned: as fast as aligned dwords (measured); odd addresses are not, hence:
    else {
        uint32_t nb0 = 0, c = a.bcn_slot - g0;
        if (g0 >= a.bcn_slot) { const uint32_t u = g0 - a.bcn_slot, j = div_ge2(u, a.bcn_div); nb0 = j + 1u; c = a.bcn_pb - (u - j * a.bcn_pb); }
        const uintptr_t p = (uintptr_t)(body + (g0 + nb0));
        const uint32_t* q = (const uint32_t*)(p & ~(uintptr_t)3);                    // the aligned dwords around the run (the stream may start at any even address: t3hip.h)
        r.w = __builtin_nontemporal_load((const u32x4*)q); r.w4 = 0;
        if (((uint32_t)p & 3u) != 0u || c < 16u) r.w4 = __builtin_nontemporal_load(q + 4);                          // (never a dword that lies wholly behind the run's last byte)
        r.x = ((uint32_t)p & 3u) | min(c, 16u) << 8;
    }
    return r;
}
template <bool BCN>
__device__ __forceinline__ void run_bytes(const Run<BCN>& r, uint32_t (&L)[4]) {
    if constexpr (!BCN) { L[0] = r.w[0]; L[1] = r.w[1]; L[2] = r.w[2]; L[3] = r.w[3]; }
    else {
        const uint32_t sh = r.x & 3u, c = r.x >> 8, dc = c >> 2, bc = c & 3u;        // dc == 4: no beacon in the run
        uint32_t F[5];
        F[0] = __builtin_amdgcn_alignbyte(r.w[1], r.w[0], sh); F[1] = __builtin_amdgcn_alignbyte(r.w[2], r.w[1], sh);
        F[2] = __builtin_amdgcn_alignbyte(r.w[3], r.w[2], sh); F[3] = __builtin_amdgcn_alignbyte(r.w4, r.w[3], sh);
        F[4] = r.w4 >> (8u * sh);                                                     // its low byte: the 17th framed byte
        const uint32_t D = dc == 0u ? F[0] : dc == 1u ? F[1] : dc == 2u ? F[2] : F[3], Dn = dc == 0u ? F[1] : dc == 1u ? F[2] : dc == 2u ? F[3] : F[4];
        const uint32_t sel = bc == 0u ? 0x04030201u : bc == 1u ? 0x04030200u : bc == 2u ? 0x04030100u : 0x04020100u;   // v_perm(S0, S1): 0..3 = S1, 4..7 = S0
        const uint32_t Mx = __builtin_amdgcn_perm(Dn, D, sel);                       // the dword the beacon sits in, without it
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i) L[i] = i < dc ? F[i] : i == dc ? Mx : __builtin_amdgcn_alignbyte(F[i + 1], F[i], 1u);
    }
}

// constants -> LDS (both kernels): band rows, counters, then the block stages' tables by the whole workgroup
template <uint32_t TCOP, uint32_t TBASE, uint32_t MT>
__device__ __forceinline__ void stage_constants(const DecFx2Args& a, const uint32_t tid, const uint32_t nthr) {
    if (tid == 0) {
        stage_band_rows(a);
        *(uint32_t*)(lds + kFx2Cnt) = 0; *(uint32_t*)(lds + kFx2Cnt + 4) = 0; *(uint32_t*)(lds + kFx2Sync) = 0; *(uint32_t*)(lds + kFx2Abort) = 0;
    }
    stage_fx2_tables<TCOP, TBASE, MT>(a, a.afrag, a.af_off, tid, nthr);
    stage_pattern_rows(a, tid);
}

// D5 (pixels) for lane slot j of a tile: four triples = 52 symbols at y_off + 52 j -> 12 pixels = 72 bytes; RGB: the inverse
// io_image.hpp bridge fused in (dequantize_ycbcr :79-84 by table, ycbcr_to_rgb :57-66 with every float step rounded on its own,
// std::lround + clamp to 0..255 = min(trunc(x + 0.5) from zero up, 255)) -> 36 bytes
template <bool RGB>
__device__ __forceinline__ void fx2_pixels12(const DecFx2Args& a, const uint32_t j, const uint32_t y_off, const uint64_t unit0, const uint32_t n_here, const uint64_t out_off = 0) {   // out_off: the frame's byte offset from a.out (batch launches)
    uint32_t D[13];
#pragma unroll
    for (int i = 0; i < 13; ++i) D[i] = *T3_LDS(const uint32_t, y_off + 52u * j + 4u * i);
    uint32_t o[18];
    px12_from_syms(D, o);
    if constexpr (RGB) {
        uint32_t w[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
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
            for (uint32_t k = 0; k < 3; ++k) { const uint32_t bi = 3u * p + k; w[bi >> 2] |= c3[k] << (8u * (bi & 3u)); }
        }
        uint8_t* g8 = (uint8_t*)a.out + out_off + (unit0 + 12ull * j) * 3u;                    // 4-byte aligned
        if (12u * j + 12u <= n_here) {
            typedef uint32_t v4u __attribute__((ext_vector_type(4), aligned(4)));
            *(v4u*)(g8) = v4u{w[0], w[1], w[2], w[3]}; *(v4u*)(g8 + 16) = v4u{w[4], w[5], w[6], w[7]}; *(uint32_t*)(g8 + 32) = w[8];
        } else {
#pragma unroll
            for (uint32_t bi = 0; bi < 36; ++bi) if (12u * j + bi / 3u < n_here) g8[bi] = (uint8_t)(w[bi >> 2] >> (8u * (bi & 3u)));
        }
    } else {
        store_px12((uint8_t*)a.out + out_off + (unit0 + 12ull * j) * 6u, o, 12u * j, n_here);
    }
}

// The pixel kernel over one frame or over a batch of equal frames in one launch (dec_frames_px): the tile loop (t3_decode_px_body.inc) is
// one text, and what differs stands here, overloaded on the argument block.  A batch's tile space is n_frames * a.n_tiles tickets; a
// ticket names a frame and a tile of it, and everything the loop derives from the tile -- band offsets, scrambler phase, block counts, the
// ragged last tile -- comes from the tile's index inside its frame; only the frame's input and output base move.  One frame: the ticket is
// the tile, no offset, and these stand for the plain expressions the kernel had in their place.
// (Scalars, no record per tile: with one, decode_fixed_px_kernel's beacon forms came out with their loop-carried copies in another order.)
__device__ __forceinline__ uint32_t px_n_tiles(const DecFx2Args& a) { return a.n_tiles; }
__device__ __forceinline__ uint32_t px_n_tiles(const DecFramesArgs& fa) { return fa.n_total; }
__device__ __forceinline__ uint32_t px_frame(const DecFramesArgs& fa, const uint32_t t) { return div_any(t, fa.div_tiles); }
__device__ __forceinline__ uint32_t px_tile(const DecFx2Args&, const uint32_t t) { return t; }                       // the tile inside its frame
__device__ __forceinline__ uint32_t px_tile(const DecFramesArgs& fa, const uint32_t t) { return t - px_frame(fa, t) * fa.a.n_tiles; }
__device__ __forceinline__ const uint8_t* px_body(const DecFx2Args&, const uint8_t* const body, const uint32_t) { return body; }   // the body of the tile's frame
__device__ __forceinline__ const uint8_t* px_body(const DecFramesArgs& fa, const uint8_t* const body, const uint32_t t) { return body + (uint64_t)px_frame(fa, t) * fa.in_stride; }
__device__ __forceinline__ uint64_t px_out_off(const DecFx2Args&, const uint32_t) { return 0; }                      // the frame's byte offset from a.out
__device__ __forceinline__ uint64_t px_out_off(const DecFramesArgs& fa, const uint32_t t) { return (uint64_t)px_frame(fa, t) * fa.out_stride; }
// the header check (launches that carry verdict words; a batch always does): one frame -- workgroup 0's; a batch -- every workgroup those
// of frames w, w + grid, .. -> verdict[2 f]
__device__ __forceinline__ bool px_header_wg(const DecFx2Args&) { return blockIdx.x == 0u; }
__device__ __forceinline__ bool px_header_wg(const DecFramesArgs&) { return true; }
__device__ __forceinline__ void px_header_check(const DecFx2Args& a, const uint32_t want, const uint32_t lane) { header_check_wave(a, want, lane); }
__device__ __forceinline__ void px_header_check(const DecFramesArgs& fa, const uint32_t want, const uint32_t lane) {
    const DecFx2Args& a = fa.a;
    for (uint32_t f = blockIdx.x; f < fa.n_frames; f += gridDim.x) {
        bool mis = false;
        if (4u * lane < a.hdr_n) {
            const uint32_t nb = min(4u, a.hdr_n - 4u * lane), mask = nb >= 4u ? 0xFFFFFFFFu : (1u << (8u * nb)) - 1u;
            mis = ((((const uint32_t*)(a.hdr_in + (uint64_t)f * fa.in_stride))[lane] ^ want) & mask) != 0u;
        }
        const bool any = __builtin_amdgcn_ballot_w64(mis) != 0;
        if (lane == 0) a.verdict[2u * f] = any ? 1u : 0u;
    }
}
// where a tile's uncorrectable blocks are counted: one frame -- the workgroup's LDS count or the caller's counter (failp); a batch -- the
// verdict word of the tile's frame at once (zeroed in front of the launch): a workgroup crosses frames, so its LDS count would not do, and
// the path is rare
__device__ __forceinline__ uint32_t* px_fail(const DecFx2Args&, uint32_t* const failp, const uint32_t) { return failp; }
__device__ __forceinline__ uint32_t* px_fail(const DecFramesArgs& fa, uint32_t* const, const uint32_t t) { return fa.a.verdict + (2u * px_frame(fa, t) + 1u); }
// ... and so a batch's finish is the done count and the re-arm of the tickets alone
__device__ __forceinline__ void px_finish(const Tickets& tk, const DecFx2Args& a, const uint32_t tid) { tk.finish(a, tid); }
__device__ __forceinline__ void px_finish(const Tickets& tk, const DecFramesArgs& fa, const uint32_t tid) {
    if (tk.dyn && tid == 0u) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (atomicAdd(fa.a.tile_ctr + 64u * tk.NC, 1u) == tk.grid - 1u)
            for (uint32_t c = 0; c <= tk.NC; ++c) __hip_atomic_store(fa.a.tile_ctr + 64u * c, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}
}  // namespace

#ifndef T3_DEC_WAVES_PER_EU
#define T3_DEC_WAVES_PER_EU 6   // <= 80 VGPRs: three 8-wave workgroups per CU
#endif
#ifdef T3_DEC_STAMPS   // diagnostic build: per-phase cycle sums of waves 0 and 4 (never in the product build)
#define T3D_STAMP(i) do { const uint64_t t_ = __builtin_amdgcn_s_memtime(); st_acc[i] += t_ - st_prev; st_prev = t_; } while (0)
#else
#define T3D_STAMP(i) do { } while (0)
#endif

// ------------------------------------------------------------------------------------------------------------------
// pixels out: producer / consumer waves
// ------------------------------------------------------------------------------------------------------------------
template <int R, bool RGB, bool BCN>
__global__ __launch_bounds__(T3_DEC_PX_THREADS, T3_DEC_WAVES_PER_EU) void decode_fixed_px_kernel(const DecFx2Args a) {
    const DecFx2Args& args = a;
#include "t3_decode_px_body.inc"
}
// a batch of equal frames (instantiated in t3_decode_frames.hip): FIXED, one k = 26 - R on all bands, 1-D, no beacon, pixels or RGB out
// (BCN: the body's parameter, and a template parameter because the body's `if constexpr (BCN)` branches name members that exist only in
// the beacon types -- they are discarded only where the condition depends on a template parameter; batches carry no beacon, only
// BCN = false is instantiated)
template <int R, bool RGB, bool BCN>
__global__ __launch_bounds__(T3_DEC_PX_THREADS, T3_DEC_WAVES_PER_EU) void dec_frames_px(const DecFramesArgs args) {
    static_assert(!BCN, "batch launches: no beacon");
    const DecFx2Args& a = args.a;
#include "t3_decode_px_body.inc"
}

}  // namespace t3
