// t3_decode_era_window.hip — a pixel WINDOW of a FIXED frame decoded with received bytes above 26 taken as erasures, written straight from
// the tiles (include/t3hip.h, "decode a window with erasures"): no scratch run, no crop launch.
//
//   decode_era_window_px<R, RGB, BCN>   decode_era_px_kernel (t3_decode_era.hip) -- its tile loop, wave roles, queues, header check, counts
//                             and tickets, the block stage of t3_decode_era_tile.h unchanged -- with another pixel stage: where
//                             fx2_pixels12 stores a lane's 12 pixels at their stream position, era_win_pixels12 stores each of them at its
//                             WINDOW position or nowhere (t3_decode_era_win_px.h: one text with the batch form).
//                             Absolute stream pixel p = first_px + (the launch's unit); row = p / fw,
//                             col = p % fw: one division per lane and 12-pixel group (the group's first pixel), then col / row stepped
//                             pixel by pixel -- a group may cross one row end or several (fw < 12).  A pixel is stored iff its unit is
//                             below the tile's n_here, y0 <= row < rows_end and x0 <= col < x0 + w, at byte
//                             ((row - y0) w + (col - x0)) (6 | 3) behind a.out: 64-bit (w h (6 | 3) may pass 2^32), p itself 32-bit (the
//                             planner bounds 9 * out_words < 2^32).  Per-pixel stores -- three 16-bit components, three RGB bytes -- are
//                             the baseline: w may be odd, so a window row starts at any 2-byte (1-byte) alignment.  Fast path: the 12
//                             pixels lie in one window row and their first byte is 4-byte aligned -> 18 (9) dword stores of the same
//                             bytes.  Window positions no stream pixel maps to are the host's (zeroed in front of the launch).
// The window scalars are read from the kernel argument where the pixel stage needs them, so none of them lives in a VGPR across the
// out-of-line era_px_block call of the consumers' queue loop.  The tile loop is this file's own text for the reason t3_decode_era.hip
// gives.  The batch form: t3_decode_era_frames_window.hip.
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
#include "t3_decode_era_tile.h"
#include "t3_decode_era_win_px.h"

namespace t3 {

// Two 8-wave workgroups per CU (up to 128 VGPRs), as decode_era_px_kernel and for its reason
#ifndef T3_DEC_ERA_WAVES_PER_EU
#define T3_DEC_ERA_WAVES_PER_EU 4
#endif
template <int R, bool RGB, bool BCN>
__global__ __launch_bounds__(T3_DEC_PX_THREADS, T3_DEC_ERA_WAVES_PER_EU) void decode_era_window_px(const DecEraWinArgs wa) {
    const DecFx2Args& a = wa.a;
    constexpr uint32_t TCOP = T3_DEC_PX_TCOP, TBASE = kFx2TPx, MT = kFx2ModPx;
    constexpr uint32_t NW = T3_DEC_PX_THREADS / 128;                                // producer waves = consumer waves
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const Tickets tk = tickets_setup(a);
    tk.first(tid);
    uint32_t* const failp = (uint32_t*)(lds + kFx2FailWg);
    if (tid == 0) { *(uint32_t*)(lds + kFx2FailWg) = 0u; *(uint32_t*)(lds + kEraCntFlagged) = 0u; *(uint32_t*)(lds + kEraCntAccepted) = 0u; }
    stage_constants<TCOP, TBASE, MT>(a, tid, blockDim.x);
    if constexpr (RGB) { if (tid < 82u) *(uint32_t*)(lds + a.dq_off + 4u * tid) = ((const uint32_t*)a.dq)[tid]; }     // yd[244] | cd[84]
    __syncthreads();
    if (blockIdx.x == 0u && wave == 2u * NW - 1u) {                                  // the header check, by a wave that starts idle
        uint32_t want = 0;                                                           // word `lane` of hx, picked here (header_check_wave, t3_decode_wg.h)
#pragma unroll
        for (uint32_t q = 0; q < 24; ++q) want = lane == q ? a.hx[q] : want;
        bool mis = false;
        if (4u * lane < a.hdr_n) {
            const uint32_t nb = min(4u, a.hdr_n - 4u * lane);
            uint32_t got = 0, mask = 0;
            for (uint32_t i = 0; i < nb; ++i) { got |= (uint32_t)a.hdr_in[4u * lane + i] << (8u * i); mask |= 0xFFu << (8u * i); }
            mis = ((got ^ want) & mask) != 0u;
        }
        const bool any = __builtin_amdgcn_ballot_w64(mis) != 0;
        if (lane == 0 && any) a.verdict[0] = 1u;
    }
    const uint8_t* body = a.in + a.hdr_syms;
    const uint32_t n_items = 9u * a.nb;
    const uint32_t units_tile = (a.TS / 13u) * 3u;                                  // pixels per tile
    uint32_t cur = blockIdx.x, nxt = tk.next(1u);                                   // this interval's tile, the next one's

    if (wave < NW) {
        // ---------------- producers: S + E1, two passes of two sets per tile and wave ----------------
        const uint32_t n = lane & 31u, h = lane >> 5;
        Geo geo[2][2]; uint32_t off0[2][2];
        const uint32_t t_off = 26u * a.nb;                                          // from a tile to the next one, in every band
#pragma unroll
        for (uint32_t p = 0; p < 2; ++p) for (uint32_t q = 0; q < 2; ++q) geo[p][q] = fx2_geo<R>(wave * 128u + p * 64u + q * 32u + n, n_items, a.nb, a.div_nb, 0u, off0[p][q]);
        auto has = [&](uint32_t pass, uint32_t set, uint32_t tile) -> bool { Geo g = geo[pass][set]; asm volatile("" : "+v"(g)); return fx2_has_block<R>(g, tile, a.n_tiles, a.nb); };
        // lanes without a block read the first bytes of the body (always there) and ignore them
        auto run_of = [&](uint32_t pass, uint32_t set, uint32_t tile) -> Run<BCN> { return load_run<BCN>(a, body, has(pass, set, tile) ? off0[pass][set] + tile * t_off + 10u * h : 0u); };
        Run<BCN> PA, PB;                                                           // the next pass's two sets, in flight
        PA.w = u32x4{0, 0, 0, 0}; PB.w = PA.w; if constexpr (BCN) { PA.x = 16u << 8; PB.x = PA.x; PA.w4 = 0; PB.w4 = 0; }
        if (cur < a.n_tiles) { PA = run_of(0, 0, cur); PB = run_of(0, 1, cur); }
        for (uint32_t k = 0; cur < a.n_tiles; ++k) {
            const uint32_t tile = cur, buf = k & 1u;
            const uint32_t y_off = a.y_off + buf * a.y_stride, q_off = a.q_off + buf * a.q_stride;
            const uint32_t u2 = 2u * mod3_u32(tile * a.nb), toff = tile * t_off;
            uint32_t raw; asm volatile("" : "=v"(raw));                                 // the counter value of lane 0's draw
#pragma unroll
            for (uint32_t pass = 0; pass < 2; ++pass) {
                uint32_t LA[4], LB[4];
                run_bytes<BCN>(PA, LA); run_bytes<BCN>(PB, LB);
                if (pass == 1u) {                                                       // the ticket for the tile after the next one (t3_decode_px_body.inc)
                    asm volatile("" : "+v"(LA[0]), "+v"(LA[1]), "+v"(LA[2]), "+v"(LA[3]), "+v"(LB[0]), "+v"(LB[1]), "+v"(LB[2]), "+v"(LB[3]));
                    if (tid == 0u && tk.dyn) raw = tk.request();
                }
                {   // the next pass's input: in flight under this pass
                    const uint32_t np = pass ^ 1u, nt = pass == 0 ? cur : nxt;
                    if (nt < a.n_tiles) { PA = run_of(np, 0, nt); PB = run_of(np, 1, nt); }
                }
                if (wave * 128u + pass * 64u < n_items) {                             // (wave-uniform) else: nothing left of the tile for this pass
                    Geo gA = geo[pass][0], gB = geo[pass][1]; asm volatile("" : "+v"(gA), "+v"(gB));
                    const Blk bA = fx2_block(gA, off0[pass][0] + toff, fx2_has_block<R>(gA, tile, a.n_tiles, a.nb), u2, y_off);
                    const Blk bB = fx2_block(gB, off0[pass][1] + toff, fx2_has_block<R>(gB, tile, a.n_tiles, a.nb), u2, y_off);
                    // the bytes-above-26 test of fx2_set, kept per block: lanes n and n + 32 hold the two halves of block n of a set
                    const uint64_t balA = __builtin_amdgcn_ballot_w64(bA.valid && rp_high13(LA, h)), balB = __builtin_amdgcn_ballot_w64(bB.valid && rp_high13(LB, h));
                    const bool ncA = (((uint32_t)balA | (uint32_t)(balA >> 32)) >> n) & 1u, ncB = (((uint32_t)balB | (uint32_t)(balB >> 32)) >> n) & 1u;
                    const Synd sA = fx2_set<R, TCOP, TBASE, MT>(bA, LA, lane, a.af_off, a.pat_off);
                    Synd sB; sB.lo = 0; sB.hi = 0;
                    if (wave * 128u + pass * 64u + 32u < n_items) sB = fx2_set<R, TCOP, TBASE, MT>(bB, LB, lane, a.af_off, a.pat_off);
                    era_px_own_blocks<R>(a.fma_off, sA, sB, bA, bB, ncA, ncB, (h ? gB : gA) & 0xFFFFu, lane, kFx2Cnt + 4u * buf, q_off);
                }
            }
            if (tid == 0u) tk.publish(buf, raw, nxt);
            barrier_lds();
            cur = nxt; nxt = tk.next(buf);
        }
        barrier_lds();                                                             // the consumers' last interval
    } else {
        // ---------------- consumers: BM / errata + D5 (into the window) of the tile the producers finished in the previous interval ----------------
        const uint32_t cw = wave - NW;
        uint32_t prev = 0;
        for (uint32_t k = 0;; ++k) {
            if (k >= 1u) {
                const uint32_t tile = prev, buf = (k - 1u) & 1u;
                const uint32_t y_off = a.y_off + buf * a.y_stride, q_off = a.q_off + buf * a.q_stride;
                const uint32_t Q = min(*(const uint32_t*)(lds + kFx2Cnt + 4u * buf), kEraQCap);
                for (uint32_t e0 = cw * 64u; e0 < Q; e0 += 64u * NW) { const uint32_t e = e0 + lane; if (e < Q) era_px_queue_entry<R, BCN>(a, body, e, q_off, y_off, tile); }
                consumer_rendezvous<NW>(k, failp, lane);                               // every patch is in LDS before any wave converts symbols
                if (tid == 64u * NW) *(uint32_t*)(lds + kFx2Cnt + 4u * buf) = 0;         // every consumer has read Q; the producers touch this counter after the barrier
                const uint32_t p_tile = wa.first_px + tile * units_tile;                 // the tile's first pixel in the stream (< 2^31)
                const uint32_t n_here = min(units_tile, wa.n_px > p_tile ? wa.n_px - p_tile : 0u);
                for (uint32_t j = cw * 64u + lane; 4u * j < a.TS / 13u; j += 64u * NW) era_win_pixels12<RGB>(wa, j, y_off, p_tile, n_here, 0ull);
            }
            barrier_lds();
            if (cur >= a.n_tiles) break;                                            // the producers had no tile in this interval: that was their closing barrier
            prev = cur; cur = nxt; nxt = tk.next(k & 1u);
        }
    }
    // the tickets re-armed by whoever finishes last; the workgroup's counts -> the verdict words (every count precedes the closing barrier)
    if (tk.dyn && tid == 0u) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (atomicAdd(a.tile_ctr + 64u * tk.NC, 1u) == tk.grid - 1u)
            for (uint32_t c = 0; c <= tk.NC; ++c) __hip_atomic_store(a.tile_ctr + 64u * c, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    if (tid < 3u) { const uint32_t v = *(const uint32_t*)(lds + (tid == 0u ? (uint32_t)kFx2FailWg : tid == 1u ? kEraCntFlagged : kEraCntAccepted)); if (v) atomicAdd(a.verdict + 1u + tid, v); }
}

#define T3_INST_ERAWB(R, BCN) template __global__ void decode_era_window_px<R, false, BCN>(const DecEraWinArgs); template __global__ void decode_era_window_px<R, true, BCN>(const DecEraWinArgs);
#define T3_INST_ERAW(R) T3_INST_ERAWB(R, false) T3_INST_ERAWB(R, true)
T3_INST_ERAW(2) T3_INST_ERAW(4) T3_INST_ERAW(6) T3_INST_ERAW(8)

}  // namespace t3
