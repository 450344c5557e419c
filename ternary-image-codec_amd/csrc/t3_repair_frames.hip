// t3_repair_frames.hip — the in-place stream repair (t3_repair.hip) over a batch of equal FIXED frames in ONE launch: frame f starts
// f * stride bytes behind frame 0, and what the launch does to it -- bytes and verdict words -- is what repair_fixed_kernel<R> does to
// that frame alone.
//
//   repair_frames_kernel<R>      repair_fixed_kernel<R> over the tile space n_frames * a.n_tiles.  Global tile t is tile t % a.n_tiles of
//                                frame t / a.n_tiles (DevDiv, as dec_frames_px); everything the loop derives from the tile -- the blocks'
//                                byte offsets, fx2_has_block, the scrambler phase -- comes from the tile's index inside its frame, only
//                                the frame's base moves (64-bit; offsets inside a frame stay 32-bit).  The walk is the grid-strided one.
//                                A step of gridDim tiles may cross any number of frame ends, so the lanes' running offsets advance by
//                                26 nb x (next local tile - this local tile), one wave-uniform product per tile, modulo 2^32 when the
//                                local tile steps back: exact for every step.  The next tile's input goes in flight under the current
//                                tile's correction phase, from the next tile's own frame.
//                                Counts: per lane, folded into LDS and flushed to the frame's verdict words when the workgroup's next
//                                tile belongs to another frame, and behind its last tile -- one global atomic per word, workgroup and
//                                frame visited, none per block.  The flush rides on the tile loop's second barrier.
//                                Tail bytes of frame f: by the workgroup that holds tile 0 of f, counted with that tile.
//   hdr_compare_frames_kernel    one workgroup per frame: verdict[nw f] = the frame's header differs from the expected symbols.
// Stores are vector byte stores.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/t3hip.h"
#include "t3_decode.h"
#include "t3_decode_fx.h"
#include "t3_decode_fx2.h"
#include "t3_decode_wg.h"
#include "t3_decode_px.h"
#include "t3_repair.h"
#include "t3_repair_blocks.h"
#include "t3_repair_tile.h"

namespace t3 {

// LDS: repair_fixed_kernel's layout; counts at kFx2Next (three words, zero between flushes)
constexpr uint32_t kRpfCnt = kFx2Next;
template <int R>
__global__ __launch_bounds__(512, T3_DEC_WAVES_PER_EU) void repair_frames_kernel(const RepairFramesArgs fa) {
    constexpr uint32_t TCOP = 32, TBASE = kFx2TSeq, MT = kFx2ModSeq;
    const DecFx2Args& a = fa.r.a;
    const uint32_t tid = threadIdx.x, nthr = blockDim.x, lane = tid & 63u, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    if (tid == 0) { *(uint32_t*)(lds + kRpfCnt) = 0; *(uint32_t*)(lds + kRpfCnt + 4) = 0; *(uint32_t*)(lds + kRpfCnt + 8) = 0; }
    stage_constants<TCOP, TBASE, MT>(a, tid, nthr);
    __syncthreads();
    const bool write = fa.r.e.write != 0u;
    const uint32_t n_items = 9u * a.nb;
    const uint32_t n = lane & 31u, h = lane >> 5;
    auto body_of = [&](const uint32_t f) -> uint8_t* { return fa.r.e.io + (uint64_t)f * fa.stride + a.hdr_syms; };
    auto frame_of = [&](const uint32_t t) -> uint32_t { return a.n_tiles <= 1u ? t : div_ge2(t, fa.div_tiles); };   // div_any, the divisor read where the loop holds it anyway
    uint32_t t = blockIdx.x, f = 0, tile = 0;                                      // global tile -> frame, tile of the frame (all wave-uniform)
    if (t < fa.n_total) { f = frame_of(t); tile = t - f * a.n_tiles; }
    uint32_t offA, offB;                                                           // running byte offsets of this wave's two blocks inside the frame (t3_decode_fx2.h)
    const Geo gA0 = fx2_geo<R>(wave * 64u + n, n_items, a.nb, a.div_nb, tile, offA), gB0 = fx2_geo<R>(wave * 64u + 32u + n, n_items, a.nb, a.div_nb, tile, offB);
    const uint32_t d_tile = 26u * a.nb;                                            // a frame's next tile: nb blocks further on in every band
    Geo gA = gA0, gB = gB0;
    auto run_of = [&](const Geo g, const uint32_t off, const uint32_t tile, const uint8_t* const body) -> Run<false> {
        return load_run<false>(a, body, fx2_has_block<R>(g, tile, a.n_tiles, a.nb) ? off + 10u * h : 0u);
    };
    Run<false> PA, PB;                                                            // this wave's two sets of the current tile, prefetched
    PA.w = u32x4{0, 0, 0, 0}; PB.w = PA.w;
    if (t < fa.n_total) { const uint8_t* const body = body_of(f); PA = run_of(gA, offA, tile, body); PB = run_of(gB, offB, tile, body); }
    RpCount cn; cn.fail = 0; cn.blocks = 0; cn.bytes = 0;
    uint32_t par = 0;
    while (t < fa.n_total) {
        uint8_t* const body = body_of(f);
        const uint32_t u2 = 2u * mod3_u32(tile * a.nb);
        asm volatile("" : "+v"(gA), "+v"(gB));                                     // opaque: keeps the unpacked pieces out of loop-long registers
        const Blk bA = fx2_block(gA, offA, fx2_has_block<R>(gA, tile, a.n_tiles, a.nb), u2, a.y_off), bB = fx2_block(gB, offB, fx2_has_block<R>(gB, tile, a.n_tiles, a.nb), u2, a.y_off);
        uint32_t LA[4], LB[4];
        run_bytes<false>(PA, LA); run_bytes<false>(PB, LB);
        // the bytes-above-26 test of fx2_set, kept per block: lanes n and n + 32 hold the two halves of block n of a set
        const uint64_t balA = __builtin_amdgcn_ballot_w64(bA.valid && rp_high13(LA, h)), balB = __builtin_amdgcn_ballot_w64(bB.valid && rp_high13(LB, h));
        const bool ncA = (((uint32_t)balA | (uint32_t)(balA >> 32)) >> n) & 1u, ncB = (((uint32_t)balB | (uint32_t)(balB >> 32)) >> n) & 1u;
        const Synd sA = fx2_set<R, TCOP, TBASE, MT>(bA, LA, lane, a.af_off, a.pat_off);
        const Synd sB = fx2_set<R, TCOP, TBASE, MT>(bB, LB, lane, a.af_off, a.pat_off);
        // the next tile's input, in flight under this tile's correction phase -- whichever frame it belongs to
        {
            const uint32_t nt = t + gridDim.x;
            if (nt < fa.n_total) {
                const uint32_t nf = frame_of(nt), ntile = nt - nf * a.n_tiles; const uint8_t* const nbody = body_of(nf);
                const uint32_t d_off = d_tile * (ntile - tile);                    // from this tile of frame f to tile ntile of frame nf: exact, modulo 2^32 when it steps back
                offA += d_off; offB += d_off;
                PA = run_of(gA, offA, ntile, nbody); PB = run_of(gB, offB, ntile, nbody);
            }
        }
        rp_own_blocks<R>(a.roots, a.fma_off, sA, sB, bA, bB, body, ncA, ncB, (h ? gB0 : gA0) & 0xFFFFu, lane, kFx2Cnt + 4u * par, a.q_off, 512u, write, cn);   // (bA / bB were built before the offsets advanced)
        barrier_lds();
        {
            const uint32_t Q = *(const uint32_t*)(lds + kFx2Cnt + 4u * par);
            for (uint32_t e0 = wave * 64u; e0 < min(Q, 512u); e0 += nthr) { const uint32_t e = e0 + lane; if (e < min(Q, 512u)) rp_queue_entry<R>(a.roots, a.fma_off, e, a.q_off, 512u, body, tile, a.nb, write, cn); }
            if (tid == 0) *(uint32_t*)(lds + kFx2Cnt + 4u * (par ^ 1u)) = 0;        // the next tile's counter (nobody touches it in this phase)
        }
        if (tile == 0) cn.bytes += rp_tail(fa.r.e, body - a.hdr_syms, tid);         // the frame's tail: once per frame, with its first tile
        // This workgroup leaves frame f (or ends): the lanes' counts -> LDS in front of the barrier, behind it three lanes move the sums to the
        // frame's verdict words and zero them.  The next fold is at least one barrier further on.
        // (the next tile's frame is worked out again here and below, not carried through the correction phase in scalar registers)
        t += gridDim.x;
        asm volatile("" : "+s"(t));
        const uint32_t nf = t < fa.n_total ? frame_of(t) : 0xFFFFFFFFu;
        const bool leave = nf != f;                                                // (workgroup-uniform; behind the last tile: no frame)
        if (leave) {
            if (cn.fail) atomicAdd((uint32_t*)(lds + kRpfCnt), cn.fail);
            if (cn.blocks) atomicAdd((uint32_t*)(lds + kRpfCnt + 4), cn.blocks);
            if (cn.bytes) atomicAdd((uint32_t*)(lds + kRpfCnt + 8), cn.bytes);
            cn.fail = 0; cn.blocks = 0; cn.bytes = 0;
        }
        barrier_lds();                                                             // the queue is free for the next tile's blocks
        if (leave && tid < 3u) {
            uint32_t* const c = (uint32_t*)(lds + kRpfCnt + 4u * tid);
            const uint32_t v = *c; *c = 0;
            if (v) atomicAdd(fa.r.e.verdict + (4u * f + 1u + tid), v);
        }
        f = nf; tile = t - f * a.n_tiles; par ^= 1u;
    }
}

template __global__ void repair_frames_kernel<2>(const RepairFramesArgs);
template __global__ void repair_frames_kernel<4>(const RepairFramesArgs);
template __global__ void repair_frames_kernel<6>(const RepairFramesArgs);
template __global__ void repair_frames_kernel<8>(const RepairFramesArgs);

// header symbols of frame blockIdx.x against the ones its configuration encodes to; writes verdict[nw f] (zeroed in front of the launch
// with the frame's other words; nw: 4, or 6 for erasure_frames_kernel of t3_repair_era_frames.hip)
__global__ __launch_bounds__(128) void hdr_compare_frames_kernel(const uint8_t* in, const uint64_t stride, const HdrExpect expect, const uint32_t n, const uint32_t nw, uint32_t* verdict) {
    __shared__ uint8_t ex[96];
    if (threadIdx.x < 96) ex[threadIdx.x] = expect.b[threadIdx.x < 96 ? threadIdx.x : 0];     // (kernel arguments are not indexed dynamically: staged)
    __syncthreads();
    const uint8_t* const hdr = in + (uint64_t)blockIdx.x * stride;
    const int diff = __syncthreads_or(threadIdx.x < n && threadIdx.x < 96 && hdr[threadIdx.x] != ex[threadIdx.x < 96 ? threadIdx.x : 0]);
    if (threadIdx.x == 0) verdict[nw * blockIdx.x] = diff ? 1u : 0u;
}

}  // namespace t3
