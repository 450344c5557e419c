// t3_repair_era.hip — repair of a FIXED coded frame in place with received bytes above 26 taken as ERASURES (include/t3hip.h, "repair
// with erasures"): a body block is accepted iff a codeword c exists with 2 e + s <= r, s = bytes of the block above 26, e = the other
// positions where c differs from the received symbol; an accepted block becomes c on the wire, any other block stays byte for byte as
// received.  s = 0 is the plain repair's rule (t3_repair.hip), and on a frame without a body byte above 26 these kernels store what
// those do.  Beacon slots, tail and dry runs: as there.
//
//   erasure_fixed_kernel<R>   the tile loop, LDS layout and matrix-core syndrome stage of repair_fixed_kernel<R> as they stand.  One
//                             difference: a block whose ballot says "holds a byte above 26" is never finished by the lane that owns it --
//                             no clean shortcut, no single-error closed form -- but queued with the tag bit (zero syndromes too; 9 x 52
//                             blocks fit the 512-entry queue).  A tagged entry re-reads its 26 wire bytes for the mask and runs the
//                             errors-and-erasures decoder of t3_rs_core.h (rs_errata) on the queue's syndromes, over the multiply-accumulate
//                             table and the small byte tables in LDS (EraField); out of line, so that its private arrays and its registers
//                             are no part of the tile loop's allocation.  Untagged entries: rp_fix_block, unchanged.  The block stage
//                             is t3_repair_era_tile.h, shared with the batch kernel (t3_repair_era_frames.hip).
//   erasure_generic_kernel    every other FIXED framing: repair_generic_kernel's map, one lane per block, rs_decode_block_erasures on
//                             (descrambled row, mask).  The correctness path; no speed is claimed for it.
//   rs_erasure_blocks_kernel  block level (t3hip_rs_decode_blocks_erasures_dev): one lane per block, no scrambler.
// Verdict words: [1..3] as the plain repair, [4] body blocks holding a byte above 26, [5] those of them accepted.
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
#include "t3_repair_era_tile.h"
#include "t3_rs_core.h"

namespace t3 {

// LDS: repair_fixed_kernel's; counts [1..3] at kFx2Next (three words), [4] and [5] at kFx2Sync and kFx2Abort (zeroed by stage_constants,
// unused by a kernel without tickets)
constexpr uint32_t kEraCnt = kFx2Next;
// Two 8-wave workgroups per CU (up to 128 VGPRs), not the plain kernel's three: the out-of-line call makes every value that lives across it
// sit in a callee-saved register, and under the 80-VGPR budget 16 of the tile loop's values went to scratch and were reloaded on the clean
// path (8K RS(26,20), clean frame: 140 us against the plain kernel's 85; without the call, as a timing build: 88; this form: 94 --
// profiles/erasures/notes.md).  -DT3_ERA_WAVES_PER_EU=6 builds the three-workgroup form.
#ifndef T3_ERA_WAVES_PER_EU
#define T3_ERA_WAVES_PER_EU 4
#endif
template <int R>
__global__ __launch_bounds__(512, T3_ERA_WAVES_PER_EU) void erasure_fixed_kernel(const RepairFxArgs ra) {
    constexpr uint32_t TCOP = 32, TBASE = kFx2TSeq, MT = kFx2ModSeq;
    const DecFx2Args& a = ra.a;
    const uint32_t tid = threadIdx.x, nthr = blockDim.x, lane = tid & 63u, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    if (tid == 0) { *(uint32_t*)(lds + kEraCnt) = 0; *(uint32_t*)(lds + kEraCnt + 4) = 0; *(uint32_t*)(lds + kEraCnt + 8) = 0; }
    stage_constants<TCOP, TBASE, MT>(a, tid, nthr);
    __syncthreads();
    uint8_t* const body = ra.e.io + a.hdr_syms;
    const bool write = ra.e.write != 0u;
    const uint32_t n_items = 9u * a.nb;
    const uint32_t n = lane & 31u, h = lane >> 5;
    uint32_t offA, offB;                                                           // running byte offsets of this wave's two blocks (t3_decode_fx2.h)
    const Geo gA0 = fx2_geo<R>(wave * 64u + n, n_items, a.nb, a.div_nb, blockIdx.x, offA), gB0 = fx2_geo<R>(wave * 64u + 32u + n, n_items, a.nb, a.div_nb, blockIdx.x, offB);
    const uint32_t d_off = 26u * a.nb * gridDim.x;
    Geo gA = gA0, gB = gB0;
    auto run_of = [&](const Geo g, const uint32_t off, const uint32_t tile) -> Run<false> { return load_run<false>(a, body, fx2_has_block<R>(g, tile, a.n_tiles, a.nb) ? off + 10u * h : 0u); };
    Run<false> PA, PB;                                                             // this wave's two sets of the current tile, prefetched
    PA.w = u32x4{0, 0, 0, 0}; PB.w = PA.w;
    if (blockIdx.x < a.n_tiles) { PA = run_of(gA, offA, blockIdx.x); PB = run_of(gB, offB, blockIdx.x); }
    RpCount cn; cn.fail = 0; cn.blocks = 0; cn.bytes = 0;
    EraCount en; en.flagged = 0; en.accepted = 0;
    uint32_t par = 0;
    for (uint32_t tile = blockIdx.x; tile < a.n_tiles; tile += gridDim.x, par ^= 1u) {
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
        {   // the next tile's input, in flight under this tile's correction phase
            const uint32_t nt = tile + gridDim.x;
            offA += d_off; offB += d_off;
            if (nt < a.n_tiles) { PA = run_of(gA, offA, nt); PB = run_of(gB, offB, nt); }
        }
        era_own_blocks<R>(a.roots, a.fma_off, sA, sB, bA, bB, body, ncA, ncB, (h ? gB0 : gA0) & 0xFFFFu, lane, kFx2Cnt + 4u * par, a.q_off, 512u, write, cn, en);   // (bA / bB were built before the offsets advanced)
        barrier_lds();
        {
            const uint32_t Q = *(const uint32_t*)(lds + kFx2Cnt + 4u * par);
            for (uint32_t e0 = wave * 64u; e0 < min(Q, 512u); e0 += nthr) { const uint32_t e = e0 + lane; if (e < min(Q, 512u)) era_queue_entry<R>(a.roots, a.fma_off, e, a.q_off, 512u, body, tile, a.nb, write, cn, en); }
            if (tid == 0) *(uint32_t*)(lds + kFx2Cnt + 4u * (par ^ 1u)) = 0;        // the next tile's counter (nobody touches it in this phase)
        }
        barrier_lds();                                                             // the queue is free for the next tile's blocks
    }
    if (blockIdx.x == 0) cn.bytes += rp_tail(ra.e, ra.e.io, tid);
    // the lanes' counts -> LDS -> the verdict words, one atomic per workgroup and word that has something to add
    if (cn.fail) atomicAdd((uint32_t*)(lds + kEraCnt), cn.fail);
    if (cn.blocks) atomicAdd((uint32_t*)(lds + kEraCnt + 4), cn.blocks);
    if (cn.bytes) atomicAdd((uint32_t*)(lds + kEraCnt + 8), cn.bytes);
    if (en.flagged) atomicAdd((uint32_t*)(lds + kFx2Sync), en.flagged);
    if (en.accepted) atomicAdd((uint32_t*)(lds + kFx2Abort), en.accepted);
    __syncthreads();
    if (tid < 3u) { const uint32_t v = *(const uint32_t*)(lds + kEraCnt + 4u * tid); if (v) atomicAdd(ra.e.verdict + 1u + tid, v); }
    else if (tid < 5u) { const uint32_t v = *(const uint32_t*)(lds + (tid == 3u ? kFx2Sync : kFx2Abort)); if (v) atomicAdd(ra.e.verdict + 1u + tid, v); }
}

template __global__ void erasure_fixed_kernel<2>(const RepairFxArgs);
template __global__ void erasure_fixed_kernel<4>(const RepairFxArgs);
template __global__ void erasure_fixed_kernel<6>(const RepairFxArgs);
template __global__ void erasure_fixed_kernel<8>(const RepairFxArgs);

// ------------------------------------------------------------------------------------------------------------------
// every other FIXED framing: one lane per block, then one lane per beacon slot
// ------------------------------------------------------------------------------------------------------------------
template <int R>
__device__ __noinline__ bool era_decode_one(const RsView& v, uint8_t* c, const uint32_t mask) { return rs_decode_block_erasures<R>(v, c, mask); }

__global__ __launch_bounds__(256) void erasure_generic_kernel(const RepairGenArgs ra) {
    const DecArgs& a = ra.d;
    __shared__ RsTables sT;
    __shared__ uint32_t sCnt[5];
    for (int i = threadIdx.x; i < (int)sizeof(RsTables); i += blockDim.x) ((uint8_t*)&sT)[i] = ((const uint8_t*)a.tab)[i];
    if (threadIdx.x < 5) sCnt[threadIdx.x] = 0;
    __syncthreads();
    const RsView v{sT.mul, sT.add, sT.neg, sT.inv, sT.exp};
    uint8_t* const body = ra.e.io + a.hdr_syms;
    const bool write = ra.e.write != 0u;
    uint32_t n_fail = 0, n_blocks = 0, n_bytes = 0, n_flag = 0, n_acc = 0;
    const uint64_t gtid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, gstride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t item = gtid; item < a.total_blocks; item += gstride) {
        int b = 0;
#pragma unroll
        for (int q = 1; q < 9; ++q) if (item >= a.band_first[q]) b = q;
        const uint64_t m = item - a.band_first[b];
        const uint32_t k = a.band_k[b];
        // v6c: band-serial body, beacon slots interleaved afterwards (the FIXED map of dec_gather_rs_kernel)
        auto wire = [&](const int i, uint64_t& q) -> uint64_t {
            q = a.band_off[b] + 26 * m + (uint64_t)i;
            uint64_t pos = q;
            if (a.beacon_on) {
                const uint64_t per = 9ull * a.period - 1u, t = q / per, rem = q - t * per;
                if (rem < 8) pos = 9 * (t * a.period) + (rem < a.slot ? rem : rem + 1);
                else { const uint64_t r2 = rem - 8; pos = 9 * (t * a.period + 1 + r2 / 9) + r2 % 9; }
            }
            return pos;
        };
        uint8_t raw[26], d0[26], c[26];
        uint32_t mask = 0;
        for (int i = 0; i < 26; ++i) {
            uint64_t q; const uint64_t pos = wire(i, q);
            raw[i] = body[pos];
            mask |= (raw[i] > 26u ? 1u : 0u) << i;
            d0[i] = rp_sub_trits(raw[i], rp_scr_state(q, a.cyc24, a.pre0, a.pre1));
            c[i] = d0[i];
        }
        bool ok;
        switch (k) {
            case 24: ok = era_decode_one<2>(v, c, mask); break;
            case 22: ok = era_decode_one<4>(v, c, mask); break;
            case 20: ok = era_decode_one<6>(v, c, mask); break;
            default: ok = era_decode_one<8>(v, c, mask); break;
        }
        if (mask) { ++n_flag; if (ok) ++n_acc; }
        if (!ok) { ++n_fail; continue; }                                           // left byte for byte as received
        uint32_t n = 0;
        for (int i = 0; i < 26; ++i) {
            // the error is the same before and after the scrambler: new wire byte = received mod 27 - (received - codeword)
            const uint8_t nv = v.S((uint8_t)(raw[i] % 27u), v.S(d0[i], c[i]));
            if (nv != raw[i]) { uint64_t q; const uint64_t pos = wire(i, q); if (write) body[pos] = nv; ++n; }
        }
        if (n) { n_bytes += n; ++n_blocks; }
    }
    for (uint64_t j = gtid; j < ra.n_bcn; j += gstride) {                           // beacon slots: the encoder's symbol
        uint8_t* const p = body + ra.bcn_first + j * ra.bcn_step;
        if (*p != (uint8_t)ra.bcn_sym) { if (write) *p = (uint8_t)ra.bcn_sym; ++n_bytes; }
    }
    if (blockIdx.x == 0) n_bytes += rp_tail(ra.e, ra.e.io, threadIdx.x);
    if (n_fail) atomicAdd(&sCnt[0], n_fail);
    if (n_blocks) atomicAdd(&sCnt[1], n_blocks);
    if (n_bytes) atomicAdd(&sCnt[2], n_bytes);
    if (n_flag) atomicAdd(&sCnt[3], n_flag);
    if (n_acc) atomicAdd(&sCnt[4], n_acc);
    __syncthreads();
    if (threadIdx.x < 5) { const uint32_t s = sCnt[threadIdx.x]; if (s) atomicAdd(ra.e.verdict + 1u + threadIdx.x, s); }
}

// block level: bytes above 26 among the 26 symbols are erasures, no scrambler.  Accepted: the codeword in place and its first k symbols
// as data; refused: both untouched.
__global__ __launch_bounds__(256) void rs_erasure_blocks_kernel(uint8_t* code, uint64_t n_blocks, int k, const RsTables* tab, uint8_t* data, uint8_t* okv) {
    __shared__ RsTables sT;
    for (int i = threadIdx.x; i < (int)sizeof(RsTables); i += blockDim.x) ((uint8_t*)&sT)[i] = ((const uint8_t*)tab)[i];
    __syncthreads();
    const RsView v{sT.mul, sT.add, sT.neg, sT.inv, sT.exp};
    const uint64_t blk = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (blk >= n_blocks) return;
    uint8_t c[26];
    uint32_t mask = 0;
    for (int i = 0; i < 26; ++i) { const uint32_t y = code[blk * 26 + i]; mask |= (y > 26u ? 1u : 0u) << i; c[i] = (uint8_t)(y % 27u); }
    bool ok;
    switch (k) {
        case 24: ok = era_decode_one<2>(v, c, mask); break;
        case 22: ok = era_decode_one<4>(v, c, mask); break;
        case 20: ok = era_decode_one<6>(v, c, mask); break;
        default: ok = era_decode_one<8>(v, c, mask); break;
    }
    if (ok) {
        for (int i = 0; i < 26; ++i) code[blk * 26 + i] = c[i];
        for (int i = 0; i < k; ++i) data[blk * k + i] = c[i];
    }
    okv[blk] = ok ? 1 : 0;
}

}  // namespace t3
