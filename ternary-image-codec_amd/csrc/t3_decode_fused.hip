// t3_decode_fused.hip — fused FIXED-mode ("v6c") decoder for gfx950: K3 syndromes + K4 Berlekamp–Massey / Chien / Forney +
// K5 symbols -> pixels|words in ONE launch, tiled like the encoder (BASELINE config 5: decode with injected trit errors).
// Replaces, for mode=FIXED / uniform k / 1-D / no beacon: descramble (OLD:938-947), per-band RS decode (OLD:963-991,
// decode_block OLD:546-662 with the Forney sign fixed), the i%9 re-merge the reference omits, symbols -> 26-trit words
// (OLD:1022-1040) and unpack_two_pixels (OLD:706-722).  Everything else goes through t3_decode_stream.hip / t3_decode.hip.
//
// Stages of a tile (9 bands x nb blocks; block stages in t3_decode_fx2.h):
//   S   a set = 32 blocks, two lanes per block: one 16-byte load per lane, one T-table read per coded symbol (descramble +
//       trit expansion), syndromes on the matrix cores (78 x 3r GF(3) product as four v_mfma_i32_32x32x32_i8), mod-3 fold by
//       byte tables, data symbols -> stream order in LDS (byte 9(mk+p)+b)
//   E1  one lane = one block: non-zero syndromes that form a geometric progression are a single error, fixed in place; the
//       other flagged blocks are appended to an LDS queue, one wave-aggregated counter update per wave (ballot + prefix count)
//   BM  full waves drain the queue: Berlekamp-Massey on a fused multiply-add table (a + x y, 27^3 bytes in LDS), Chien search
//       by table (root mask per locator, global memory), Forney, <= t bytes patched
//   D5  pixels: one lane = four triples, 13 aligned dwords of symbols -> 12 pixels with packed 16-bit ops -> 72 bytes stored
//       straight to memory;  raw words: 26 symbols -> 3 words, staged in LDS, copied out with 16-byte coalesced stores.
//
// decode_fixed_px_kernel (pixels): every stage is a chain of dependent LDS reads (the correction alone is ~35 levels), so a
// workgroup that runs them one after the other spends most of a tile waiting.  Waves 0-3 (producers) therefore run S + E1 of tile
// k while waves 4-7 (consumers) run BM + D5 of tile k-1 on the other symbol buffer / queue: one workgroup barrier per tile, a
// four-wave rendezvous (LDS counter) between BM and D5.  The producers issue no stores and the consumers no streaming loads,
// so the input loads (issued one pass ahead) never wait behind store acknowledgements.
// decode_fixed_kernel (raw words): the same stages one after the other.
// The frame around the stages -- constants to LDS, tile tickets, verdict words, header check, consumer rendezvous, the 72-byte pixel
// store -- is t3_decode_wg.h, shared with t3_decode_uep.hip; small device helpers: t3_devutil.h.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/t3hip.h"
#include "t3_decode.h"
#include "t3_decode_fx.h"
#include "t3_decode_fx2.h"
#include "t3_decode_wg.h"
#include "t3_decode_px.h"

namespace t3 {
// (a lane's coded run, constants -> LDS, the pixel output stage, and decode_fixed_px_kernel itself: t3_decode_px.h)

// ------------------------------------------------------------------------------------------------------------------
// raw words out: the phases one after the other
// ------------------------------------------------------------------------------------------------------------------
template <int R, bool BCN>
__global__ __launch_bounds__(512, T3_DEC_WAVES_PER_EU) void decode_fixed_kernel(const DecFx2Args a) {
    constexpr uint32_t TCOP = 32, TBASE = kFx2TSeq, MT = kFx2ModSeq;
    const uint32_t tid = threadIdx.x, nthr = blockDim.x, lane = tid & 63u, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    stage_constants<TCOP, TBASE, MT>(a, tid, nthr);
    __syncthreads();
    const uint8_t* body = a.in + a.hdr_syms;
    const uint32_t n_items = 9u * a.nb;
    const uint32_t units_tile = (a.TS / 26u) * 3u;                                  // words per tile
    const uint32_t n = lane & 31u, h = lane >> 5;
    uint32_t offA, offB;                                                           // running byte offsets of this wave's two blocks (t3_decode_fx2.h)
    const Geo gA0 = fx2_geo<R>(wave * 64u + n, n_items, a.nb, a.div_nb, blockIdx.x, offA), gB0 = fx2_geo<R>(wave * 64u + 32u + n, n_items, a.nb, a.div_nb, blockIdx.x, offB);
    const uint32_t d_off = 26u * a.nb * gridDim.x;
    Geo gA = gA0, gB = gB0;
    auto run_of = [&](const Geo g, const uint32_t off, const uint32_t tile) -> Run<BCN> { return load_run<BCN>(a, body, fx2_has_block<R>(g, tile, a.n_tiles, a.nb) ? off + 10u * h : 0u); };
    Run<BCN> PA, PB;                                                               // this wave's two sets of the current tile, prefetched
    PA.w = u32x4{0, 0, 0, 0}; PB.w = PA.w; if constexpr (BCN) { PA.x = 16u << 8; PB.x = PA.x; PA.w4 = 0; PB.w4 = 0; }
    if (blockIdx.x < a.n_tiles) { PA = run_of(gA, offA, blockIdx.x); PB = run_of(gB, offB, blockIdx.x); }
    uint32_t par = 0;
    for (uint32_t tile = blockIdx.x; tile < a.n_tiles; tile += gridDim.x, par ^= 1u) {
        const uint32_t u2 = 2u * mod3_u32(tile * a.nb);
        asm volatile("" : "+v"(gA), "+v"(gB));                                     // opaque: keeps the unpacked pieces out of loop-long registers
        const Blk bA = fx2_block(gA, offA, fx2_has_block<R>(gA, tile, a.n_tiles, a.nb), u2, a.y_off), bB = fx2_block(gB, offB, fx2_has_block<R>(gB, tile, a.n_tiles, a.nb), u2, a.y_off);
        uint32_t LA[4], LB[4];
        run_bytes<BCN>(PA, LA); run_bytes<BCN>(PB, LB);
        const Synd sA = fx2_set<R, TCOP, TBASE, MT>(bA, LA, lane, a.af_off, a.pat_off);
        const Synd sB = fx2_set<R, TCOP, TBASE, MT>(bB, LB, lane, a.af_off, a.pat_off);
        {   // the next tile's input, in flight under this tile's correction phase
            const uint32_t nt = tile + gridDim.x;
            offA += d_off; offB += d_off;
            if (nt < a.n_tiles) { PA = run_of(gA, offA, nt); PB = run_of(gB, offB, nt); }
        }
        fx2_own_blocks<R>(a.roots, a.fma_off, a.fail, sA, sB, bA, bB, (h ? gB0 : gA0) & 0xFFFFu, lane, kFx2Cnt + 4u * par, a.q_off, 512u);   // (bA / bB were built before the offsets advanced)
        barrier_lds();
        {
            const uint32_t Q = *(const uint32_t*)(lds + kFx2Cnt + 4u * par);
            for (uint32_t e0 = wave * 64u; e0 < Q; e0 += nthr) { const uint32_t e = e0 + lane; if (e < Q) fx2_queue_entry<R>(a.roots, a.fma_off, a.fail, e, a.q_off, 512u, a.y_off); }
            if (tid == 0) *(uint32_t*)(lds + kFx2Cnt + 4u * (par ^ 1u)) = 0;        // the next tile's counter (nobody touches it in this phase)
        }
        barrier_lds();
        // the loads are waited for BEFORE this tile's stores are issued (vmcnt completes in order, stores count too): they have had
        // the correction phase to land, and the wait does not cover the acknowledgement of stores issued a moment ago
        asm volatile("" : "+v"(PA.w), "+v"(PB.w));
        if constexpr (BCN) asm volatile("" : "+v"(PA.x), "+v"(PB.x), "+v"(PA.w4), "+v"(PB.w4));
        const uint64_t unit0 = (uint64_t)tile * units_tile;
        const uint32_t n_here = (uint32_t)min((uint64_t)units_tile, a.n_units > unit0 ? a.n_units - unit0 : 0ull);
        const uint32_t ng = a.TS / 26u;                                            // groups of 26 symbols -> 3 words (OLD:1022-1040)
        for (uint32_t j = tid; j < ng; j += nthr) words3_from_syms(a.y_off + 26u * j, a.o_off + 27u * j);
        __syncthreads();
        copy_out_lds((uint8_t*)a.out + unit0 * 9u, a.o_off, n_here * 9u, tid, nthr);   // tile starts are only 8-byte aligned
        barrier_lds();
    }
}

#define T3_INST_DECB(R, BCN) template __global__ void decode_fixed_kernel<R, BCN>(const DecFx2Args); template __global__ void decode_fixed_px_kernel<R, false, BCN>(const DecFx2Args); \
    template __global__ void decode_fixed_px_kernel<R, true, BCN>(const DecFx2Args);
#define T3_INST_DEC(R) T3_INST_DECB(R, false) T3_INST_DECB(R, true)
T3_INST_DEC(2) T3_INST_DEC(4) T3_INST_DEC(6) T3_INST_DEC(8)

}  // namespace t3
