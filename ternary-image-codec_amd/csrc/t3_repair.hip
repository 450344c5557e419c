// t3_repair.hip — repair of a FIXED-mode ("v6c") coded frame in place: every body block that lies within t symbols of a codeword is
// rewritten to that codeword on the wire -- data and parity positions alike, as canonical bytes 0..26 -- and every other byte of an
// accepted block above 26 to its residue mod 27; an uncorrectable block stays byte for byte as received; beacon slots get the encoder's
// symbol, the bytes behind the body up to the frame's last word become 0.  No pixel is produced and no second buffer written.
//
//   repair_fixed_kernel<R>   one k = 26 - R on all bands, no beacon.  1-D and 2-D frames alike: the interleave permutes DATA symbols ahead
//                            of the band split (OLD:1083-1088), the blocks on the wire are the same band-serial RS blocks either way, and a
//                            codeword is a codeword whatever its data means (proven on the oracle in tests/test_repair_semantics.py).
//                            Block stages of the fused decoder as they stand (t3_decode_fx2.h: fx2_geo / fx2_block / load_run<false>, fx2_set
//                            for the syndromes on the matrix cores -- its symbol-buffer writes land in a scratch row nobody reads --, the
//                            single-error closed form, fx2_correct behind the ballot queue); new is where a correction lands
//                            (t3_repair_blocks.h): global byte body + off + pos for every pos in 0..25, the received byte mod 27 minus the
//                            magnitude through the multiply-accumulate table -- the error value is the same before and after the scrambler.
//                            The kernel reads the coded bytes once and stores almost nothing, so there is no store traffic for the input
//                            loads to queue behind and no consumer to overlap: the tile loop is a plain strided loop over a persistent grid,
//                            as in decode_fixed_kernel, without the ticket machinery.  Stores are vector byte stores.
//   repair_generic_kernel    every other FIXED framing (per-band k up to four codes, with or without a beacon): one lane per block through
//                            the FIXED index map of dec_gather_rs_kernel (band-serial plus beacon skip), decision by t3_rs_core.h.  The
//                            correctness path; no speed is claimed for it.
// Either launch writes the tail bytes (workgroup 0) and adds its counts to the verdict words.
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

// LDS: the raw-word decoder's [hdr 0][fold tables 3072][T32 3584][FMA][A operand][pattern rows][Y][Q]; counts at kFx2Next (three words)
constexpr uint32_t kRpCnt = kFx2Next;
template <int R>
__global__ __launch_bounds__(512, T3_DEC_WAVES_PER_EU) void repair_fixed_kernel(const RepairFxArgs ra) {
    constexpr uint32_t TCOP = 32, TBASE = kFx2TSeq, MT = kFx2ModSeq;
    const DecFx2Args& a = ra.a;
    const uint32_t tid = threadIdx.x, nthr = blockDim.x, lane = tid & 63u, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    if (tid == 0) { *(uint32_t*)(lds + kRpCnt) = 0; *(uint32_t*)(lds + kRpCnt + 4) = 0; *(uint32_t*)(lds + kRpCnt + 8) = 0; }
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
        rp_own_blocks<R>(a.roots, a.fma_off, sA, sB, bA, bB, body, ncA, ncB, (h ? gB0 : gA0) & 0xFFFFu, lane, kFx2Cnt + 4u * par, a.q_off, 512u, write, cn);   // (bA / bB were built before the offsets advanced)
        barrier_lds();
        {
            const uint32_t Q = *(const uint32_t*)(lds + kFx2Cnt + 4u * par);
            for (uint32_t e0 = wave * 64u; e0 < min(Q, 512u); e0 += nthr) { const uint32_t e = e0 + lane; if (e < min(Q, 512u)) rp_queue_entry<R>(a.roots, a.fma_off, e, a.q_off, 512u, body, tile, a.nb, write, cn); }
            if (tid == 0) *(uint32_t*)(lds + kFx2Cnt + 4u * (par ^ 1u)) = 0;        // the next tile's counter (nobody touches it in this phase)
        }
        barrier_lds();                                                             // the queue is free for the next tile's blocks
    }
    if (blockIdx.x == 0) cn.bytes += rp_tail(ra.e, ra.e.io, tid);
    // the lanes' counts -> LDS -> the verdict words, one atomic per workgroup and word that has something to add
    if (cn.fail) atomicAdd((uint32_t*)(lds + kRpCnt), cn.fail);
    if (cn.blocks) atomicAdd((uint32_t*)(lds + kRpCnt + 4), cn.blocks);
    if (cn.bytes) atomicAdd((uint32_t*)(lds + kRpCnt + 8), cn.bytes);
    __syncthreads();
    if (tid < 3u) { const uint32_t v = *(const uint32_t*)(lds + kRpCnt + 4u * tid); if (v) atomicAdd(ra.e.verdict + 1u + tid, v); }
}

template __global__ void repair_fixed_kernel<2>(const RepairFxArgs);
template __global__ void repair_fixed_kernel<4>(const RepairFxArgs);
template __global__ void repair_fixed_kernel<6>(const RepairFxArgs);
template __global__ void repair_fixed_kernel<8>(const RepairFxArgs);

// ------------------------------------------------------------------------------------------------------------------
// every other FIXED framing: one lane per block, then one lane per beacon slot
// ------------------------------------------------------------------------------------------------------------------
template <int R>
__device__ __noinline__ bool rp_decode_one(const RsView& v, uint8_t* c) { return rs_decode_block<R>(v, c, true); }

__global__ __launch_bounds__(256) void repair_generic_kernel(const RepairGenArgs ra) {
    const DecArgs& a = ra.d;
    __shared__ RsTables sT;
    __shared__ uint32_t sCnt[3];
    for (int i = threadIdx.x; i < (int)sizeof(RsTables); i += blockDim.x) ((uint8_t*)&sT)[i] = ((const uint8_t*)a.tab)[i];
    if (threadIdx.x < 3) sCnt[threadIdx.x] = 0;
    __syncthreads();
    const RsView v{sT.mul, sT.add, sT.neg, sT.inv, sT.exp};
    uint8_t* const body = ra.e.io + a.hdr_syms;
    const bool write = ra.e.write != 0u;
    uint32_t n_fail = 0, n_blocks = 0, n_bytes = 0;
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
        for (int i = 0; i < 26; ++i) {
            uint64_t q; const uint64_t pos = wire(i, q);
            raw[i] = body[pos];
            d0[i] = rp_sub_trits(raw[i], rp_scr_state(q, a.cyc24, a.pre0, a.pre1));
            c[i] = d0[i];
        }
        bool ok;
        switch (k) {
            case 24: ok = rp_decode_one<2>(v, c); break;
            case 22: ok = rp_decode_one<4>(v, c); break;
            case 20: ok = rp_decode_one<6>(v, c); break;
            default: ok = rp_decode_one<8>(v, c); break;
        }
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
    __syncthreads();
    if (threadIdx.x < 3) { const uint32_t s = sCnt[threadIdx.x]; if (s) atomicAdd(ra.e.verdict + 1u + threadIdx.x, s); }
}

}  // namespace t3
