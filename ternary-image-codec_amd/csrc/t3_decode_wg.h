// t3_decode_wg.h — the workgroup frame of the one-launch FIXED decoders: what decode_fixed_px_kernel (t3_decode_fused.hip) and
// decode_uep_px_kernel (t3_decode_uep.hip) do around their block stages, and the pieces of it decode_fixed_kernel,
// decode_stream_kernel and emit_stream_kernel (t3_decode_stream.hip) use.  Templates over the argument block: DecFx2Args and
// DecUepArgs (t3_decode.h) name the shared fields alike.
//   constants -> LDS      stage_band_rows, stage_fx2_tables, stage_pattern_rows
//   tile tickets          Tickets: set-up, first(), request(), publish() / next(), finish() -- separate calls, because WHERE each
//                         one stands in the kernel decides which loads its s_waitcnt vmcnt covers
//   verdict               header_check_wave; failures are counted in LDS (kFx2FailWg) and added to the launch's counter in finish()
//   consumer waves        consumer_rendezvous
//   pixels out            store_px12
// The encoder's tickets (EncTickets, t3_encode.h) are drawn by the last wave through an LDS slot of their own and have a static second
// round: another protocol, not folded in here.
#pragma once
#include "t3_decode_fx.h"
#include "t3_host.hpp"

namespace t3 {
namespace {

// the nine band rows -> lds + 16 b (one thread)
template <class A>
__device__ __forceinline__ void stage_band_rows(const A& a) {
#pragma unroll
    for (int b = 0; b < 9; ++b) { Row r; r.blocks = a.band_blocks[b]; r.boff6 = a.band_boff6[b]; r.body_off = a.band_body_off[b]; *(Row*)(lds + 16 * b) = r; }
}

// The block stages' constants (t3_decode_fx2.h) -> LDS, by the whole workgroup: byte tables, fold tables at MT, TCOP copies of T at TBASE,
// multiply-accumulate table, the A operand `afrag` at af_off (three steps: 3072 bytes).
// afrag, af_off: fields of the argument block, by reference -- read where they are used, as the kernels did; by value they are loaded
// once at the top, and that alone reschedules decode_fixed_px_kernel's tile loop
template <uint32_t TCOP, uint32_t TBASE, uint32_t MT, class A>
__device__ __forceinline__ void stage_fx2_tables(const A& a, const uint32_t* const& afrag, const uint32_t& af_off, const uint32_t tid, const uint32_t nthr) {
    for (uint32_t i = tid * 16u; i < (uint32_t)kFx2SmallBytes; i += nthr * 16u) *(uint4*)(lds + kFx2Small + i) = *(const uint4*)(a.small + i);
    for (uint32_t i = tid * 16u; i < (uint32_t)kFx2ModBytes; i += nthr * 16u) *(uint4*)(lds + MT + i) = *(const uint4*)(a.small + kFx2SmallBytes + i);
    for (uint32_t i = tid * 16u; i < 3u * 27u * 4u * TCOP; i += nthr * 16u) *(uint4*)(lds + TBASE + i) = *(const uint4*)((const uint8_t*)a.ttab + i);
    for (uint32_t i = tid * 16u; i < 19696u; i += nthr * 16u) *(uint4*)(lds + a.fma_off + i) = *(const uint4*)(a.fma + i);
    for (uint32_t i = tid * 16u; i < 3072u; i += nthr * 16u) *(uint4*)(lds + af_off + i) = *(const uint4*)((const uint8_t*)afrag + i);
}
// ... and the scrambler pattern rows (t3_decode_fx2.h, fx2_set), by one thread of the second wave: constant indices only.  Its own call,
// because the two kernels issue it on different sides of the table loads
template <class A>
__device__ __forceinline__ void stage_pattern_rows(const A& a, const uint32_t tid) {
    if (tid == 64u) {
#pragma unroll
        for (int i = 0; i < 48; ++i) *(uint32_t*)(lds + a.pat_off + 4 * i) = a.pat[i];
    }
}

// Tiles are handed out by tickets, as in the encoder (t3_encode.h): the workgroups of a CU progress at different speeds (a static
// stride left the slowest workgroup 20 % behind the mean: stamp build, profiles/r03/notes.md).  Workgroup w starts with tile w; every
// further tile is drawn from a counter -- one per class (index mod n_classes: a memory-side atomic serves ~11 ns per draw, too slow
// for one counter and 15 k tiles).  The id of tile k + 2 is drawn by lane 0 of wave 0 during tile k and handed to all waves through
// an LDS slot per barrier parity (kFx2Next); an id >= n_tiles ends the workgroup.  a.tile_ctr == nullptr: static stride.
struct Tickets {
    bool dyn; uint32_t grid, NC, cls, wgc; uint32_t* ctr;      // wgc: workgroups (= static first tiles) of this class
    // tile 1 (slot of parity 1; read behind the kernel's first barrier)
    __device__ __forceinline__ void first(const uint32_t tid) const { if (tid == 0) *(uint32_t*)(lds + kFx2Next + 4u) = dyn ? cls + NC * (wgc + atomicAdd(ctr, 1u)) : blockIdx.x + grid; }
    // the bare draw: a returning atomic whose result is waited for where publish() uses it, a pass later (the decoders are built
    // without the compiler's atomic optimiser, which would read the counter back at once)
    __device__ __forceinline__ uint32_t request() const { return atomicAdd(ctr, 1u); }
    // by the thread that drew.  raw: request()'s value (dyn); nxt: the next interval's tile (static stride).  By reference, and the
    // `if (tid == 0u)` stays with the caller: a by-value `raw` is a copy of the draw's result in front of that branch, which waits for the draw
    __device__ __forceinline__ void publish(const uint32_t buf, const uint32_t& raw, const uint32_t& nxt) const {
        *(uint32_t*)(lds + kFx2Next + 4u * buf) = dyn ? cls + NC * (wgc + raw) : nxt + grid;
    }
    __device__ __forceinline__ uint32_t next(const uint32_t buf) const { return __builtin_amdgcn_readfirstlane(*(const uint32_t*)(lds + kFx2Next + 4u * buf)); }
    // Re-arm the counters for the next launch on this stream: whoever finishes last.  With verdict words the workgroup's failures go
    // from LDS to the launch's counter first (every count precedes the tile loops' closing barrier), and the last workgroup moves that
    // counter to verdict[1] (every other workgroup's counts precede its done count) and re-zeroes it.
    template <class A>
    __device__ __forceinline__ void finish(const A& a, const uint32_t tid) const {
        if (dyn && tid == 0u) {
            if (a.verdict) { const uint32_t wgf = *(const uint32_t*)(lds + kFx2FailWg); if (wgf) atomicAdd(a.fail, wgf); }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            if (atomicAdd(a.tile_ctr + 64u * NC, 1u) == grid - 1u) {
                if (a.verdict) a.verdict[1] = atomicExch(a.fail, 0u);                    // uncorrectable blocks of the whole launch
                for (uint32_t c = 0; c <= NC; ++c) __hip_atomic_store(a.tile_ctr + 64u * c, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
};
template <class A>
__device__ __forceinline__ Tickets tickets_setup(const A& a) {
    Tickets t;
    t.grid = gridDim.x; t.dyn = a.tile_ctr != nullptr;
    t.NC = t.dyn ? a.n_classes : 1u; t.cls = blockIdx.x % t.NC;
    t.wgc = (t.grid - t.cls + t.NC - 1u) / t.NC;
    t.ctr = a.tile_ctr + 64u * t.cls;
    return t;
}

// The header check (hdr_compare_kernel's job) by one wave -- the last consumer wave of workgroup 0, which starts idle: the stream's first
// hdr_n bytes against the 24 words of hx -> verdict[0]
// `want`: word `lane` of hx.  The kernel picks it itself, with a 24-step select loop in its own body: that loop indexes the argument
// block by a counter, and while it does the compiler reads every argument from the kernel-argument segment where it is used.  With
// the loop in a function that takes the block by reference, the block is copied to registers whole at the kernel's entry instead
// (every argument loaded up front; decode_fixed_px_kernel then spills 71 scalar registers and reloads them inside its tile loop).
template <class A>
__device__ __forceinline__ void header_check_wave(const A& a, const uint32_t want, const uint32_t lane) {
    bool mis = false;
    if (4u * lane < a.hdr_n) {
        const uint32_t nb = min(4u, a.hdr_n - 4u * lane), mask = nb >= 4u ? 0xFFFFFFFFu : (1u << (8u * nb)) - 1u;
        mis = ((((const uint32_t*)a.hdr_in)[lane] ^ want) & mask) != 0u;
    }
    const bool any = __builtin_amdgcn_ballot_w64(mis) != 0;
    if (lane == 0) a.verdict[0] = any ? 1u : 0u;
}

// Rendezvous number `target` (1, 2, ..) of the NW consumer waves: every wave's LDS writes are done before any wave goes on.  An LDS
// counter (kFx2Sync, zero at the start) that only grows; the spin is bounded (never seen to run out; a bound, not a path): the wave
// that gives up sets kFx2Abort and makes the launch fail.
template <uint32_t NW>
__device__ __forceinline__ void consumer_rendezvous(const uint32_t target, uint32_t* const failp, const uint32_t lane) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    uint32_t* const sync = (uint32_t*)__builtin_assume_aligned(lds + kFx2Sync, 4);
    if (lane == 0) __hip_atomic_fetch_add(sync, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    uint32_t spins = 0;
    while (__hip_atomic_load(sync, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < NW * target) {
        __builtin_amdgcn_s_sleep(1);
        if (++spins > (1u << 22)) { if (lane == 0) { *(uint32_t*)(lds + kFx2Abort) = 1u; atomicAdd(failp, 1u << 20); } break; }
    }
}

// 12 pixels = 18 dwords (px12_from_syms) -> 72 bytes at g (8-byte aligned): pixels p0 .. p0 + 11 of the n_px there are; the ones past
// the end -- the frame's last pixels -- are left out, per 16-bit component.  (decode_fixed_px_kernel and emit_stream_kernel; the UEP
// kernel's 2-byte-aligned form stays in that kernel.)
__device__ __forceinline__ void store_px12(uint8_t* const g, const uint32_t (&o)[18], const uint32_t p0, const uint32_t n_px) {
    if (p0 + 12u <= n_px) {
#pragma unroll
        for (int d = 0; d < 4; ++d) { U128a<8> w; w.v = u32x4{o[4 * d], o[4 * d + 1], o[4 * d + 2], o[4 * d + 3]}; *(U128a<8>*)(g + 16 * d) = w; }
        U64a<8> w2; w2.v = u32x2{o[16], o[17]}; *(U64a<8>*)(g + 64) = w2;
    } else {
#pragma unroll
        for (uint32_t hh = 0; hh < 36; ++hh)
            if (p0 + hh / 3u < n_px) *(uint16_t*)(g + 2u * hh) = (uint16_t)(o[hh >> 1] >> (16u * (hh & 1u)));
    }
}

}  // namespace
}  // namespace t3
