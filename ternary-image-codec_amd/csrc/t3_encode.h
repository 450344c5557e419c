// t3_encode.h — K2, the fused encoder: pixels | raw words | RGB -> coded band-serial body (encode_profile_from_raw OLD:1043-1169) in one
// persistent launch.  encode_body is the tile loop; its pieces stand in front of it, phase 1 in t3_enc_convert.h, phase 2 in
// t3_enc_parity.h.  Included by one translation unit per front end (t3_encode_px.hip, t3_encode_words.hip, t3_encode_rgb.hip), which
// instantiate the kernels enc_kernel() (t3_api_encode.cpp) picks from.
//   constants -> LDS      stage_enc_header, write_frame_ends
//   a tile's input        TileIn / tile_in, first_group, end_group, stage_tile
//   tile tickets          EncTickets: separate calls, each at the place in the tile its wait belongs to
//   2-D passes            reverse_rows_placed, reverse_rows16, permute_rows (each returns where phase 2 finds the symbols)
//   raw words in 2-D      phase1_sync_rows (the chunk loop stays in encode_body)
//   phase 2               enc_regeo, phase2
//   diagnostic stamps     EncStamps (-DT3_STAMPS; empty in the product build)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "t3_device.h"
#include "t3_devutil.h"
#include "t3_enc_convert.h"
#include "t3_enc_parity.h"

namespace t3 {

// workgroup barrier that waits for this wave's LDS traffic only: unlike __syncthreads() it leaves the LDS-DMA prefetch
// of the next tile (and the previous tile's global stores) in flight
// ... and the one at the top of a tile, which also drains vmcnt: the prefetched input has landed for every wave
__device__ __forceinline__ void barrier_all() { asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
// Top-of-tile barrier: vmcnt completes in order and the LDS-DMA prefetch of this tile was issued BEFORE the previous tile's
// `younger` global stores, so waiting until at most `younger` operations are outstanding is exactly "the input has landed"
// without also waiting for those stores to be acknowledged.
__device__ __forceinline__ void barrier_input(uint32_t younger) {
    switch (younger) {
        case 1: asm volatile("s_waitcnt vmcnt(1) lgkmcnt(0)\n\ts_barrier" ::: "memory"); break;
        case 2: asm volatile("s_waitcnt vmcnt(2) lgkmcnt(0)\n\ts_barrier" ::: "memory"); break;
        case 3: asm volatile("s_waitcnt vmcnt(3) lgkmcnt(0)\n\ts_barrier" ::: "memory"); break;
        case 4: asm volatile("s_waitcnt vmcnt(4) lgkmcnt(0)\n\ts_barrier" ::: "memory"); break;
        case 7: asm volatile("s_waitcnt vmcnt(7) lgkmcnt(0)\n\ts_barrier" ::: "memory"); break;
        case 8: asm volatile("s_waitcnt vmcnt(8) lgkmcnt(0)\n\ts_barrier" ::: "memory"); break;
        default: barrier_all(); break;
    }
}

// Diagnostic build (-DT3_STAMPS): per-phase cycle sums of wave 0, written to a.dbg by thread 0 (stamps_report, t3_api_encode.cpp).  In the
// product build every member is empty.
#ifdef T3_STAMPS
struct EncStamps {
    uint64_t entry, first, acc[6], prev, t0, rt0;
    __device__ __forceinline__ void enter() { entry = __builtin_amdgcn_s_memtime(); first = 0; }   // kernel entry -> the first tile's input has landed (wave 0)
    __device__ __forceinline__ void arm() { for (int i = 0; i < 6; ++i) acc[i] = 0; prev = __builtin_amdgcn_s_memtime(); t0 = prev; rt0 = __builtin_amdgcn_s_memrealtime(); }
    __device__ __forceinline__ void mark(const int i) { const uint64_t t_ = __builtin_amdgcn_s_memtime(); acc[i] += t_ - prev; prev = t_; }
    __device__ __forceinline__ void landed() { if (!first) first = prev - entry; }
    __device__ __forceinline__ void report(const EncArgs& a, const uint32_t tid) const {
        if (tid == 0 && a.dbg) {
            uint64_t* d = a.dbg + 16ull * blockIdx.x;
            d[8] = __builtin_amdgcn_s_getreg(31 << 11 | 4); d[9] = __builtin_amdgcn_s_getreg(31 << 11 | 20);   // HW_ID, XCC_ID
            d[0] = acc[0]; d[1] = acc[1]; d[2] = acc[2] + acc[3]; d[3] = rt0; d[10] = acc[3]; d[11] = first;
            d[4] = __builtin_amdgcn_s_memtime() - t0; d[5] = __builtin_amdgcn_s_memrealtime() - rt0; d[6] = acc[4]; d[7] = acc[5];
        }
    }
};
#else
struct EncStamps {
    __device__ __forceinline__ void enter() {}
    __device__ __forceinline__ void arm() {}
    __device__ __forceinline__ void mark(const int) {}
    __device__ __forceinline__ void landed() {}
    __device__ __forceinline__ void report(const EncArgs&, const uint32_t) const {}
};
#endif

// per-band geometry and wave roles -> LDS header (kernel arguments must not be indexed dynamically: that would
// force a private copy of the whole argument block); LUT images -> LDS once per (persistent) workgroup; FE_RGB: the chroma quantiser table
template <int FE, int RSEL>
__device__ __forceinline__ void stage_enc_header(const EncArgs& a, const uint32_t tid, const uint32_t nthr) {
    if (tid == 0) {
#pragma unroll
        for (int b = 0; b < 9; ++b) {
            BandRow r; r.k = a.band_k[b]; r.nbt = a.band_nb_tile[b]; r.blocks = a.band_blocks[b]; r.lut_off = a.band_lut_off[b];
            r.pad_ = 0; r.boff6 = a.band_boff6[b]; r.body_off = a.band_body_off[b];
            *(BandRow*)(lds + kHdrBandRow * b) = r;
        }
#pragma unroll
        for (int b = 0; b < 10; ++b) *(uint32_t*)(lds + kHdrBandFirst + 4 * b) = a.band_first[b];
#pragma unroll
        for (int i = 0; i < 12; ++i) *(uint32_t*)(lds + kHdrScr + 4 * i) = a.scr[i];
        if constexpr (RSEL == 1) {                                            // UEP group records and the set table
#pragma unroll
            for (int gi = 0; gi < kMaxGrp; ++gi) {
                uint32_t* gp = (uint32_t*)(lds + kHdrGrp + kHdrGrpStride * gi);
                gp[0] = a.grp[gi].nb; gp[1] = a.grp[gi].div_nb.mul; gp[2] = a.grp[gi].div_nb.sh; gp[3] = a.grp[gi].div_nb.d;
                gp[4] = a.grp[gi].n_items; gp[5] = a.grp[gi].r; gp[9] = a.grp[gi].afrag_off;
#pragma unroll
                for (int q = 0; q < 3; ++q) gp[6 + q] = (uint32_t)a.grp[gi].bands[4 * q] | (uint32_t)a.grp[gi].bands[4 * q + 1] << 8 | (uint32_t)a.grp[gi].bands[4 * q + 2] << 16 | (uint32_t)a.grp[gi].bands[4 * q + 3] << 24;
#pragma unroll
                for (int q = 0; q < 12; ++q) gp[12 + q] = a.grp[gi].scr[q];
            }
#pragma unroll
            for (int q = 0; q < kMaxSets; ++q) *(uint32_t*)(lds + kHdrSets + 4 * q) = a.set_tab[q];
        }
    }
    for (uint32_t i = tid * 16u; i < a.lut_bytes; i += nthr * 16u)
        *(uint4*)(lds + (RSEL == 1 ? kLdsHdrUep : kLdsHdr) + i) = *(const uint4*)((const uint8_t*)a.lut_img + i);

    if constexpr (FE == FE_RGB) { if (tid < 64u) *(uint32_t*)(lds + a.qt_off + 4u * tid) = ((const uint32_t*)a.qt)[tid]; }
}
// header symbols + zero tail (OLD:1159-1167), and the framed bytes behind the last body byte (BCN), by workgroup 0
template <bool BCN>
__device__ __forceinline__ void write_frame_ends(const EncArgs& a, const uint32_t tid) {
    if (blockIdx.x == 0 && a.frame_out) {
        if (tid == 0) {                                                      // constant indices only (see above)
#pragma unroll
            for (uint32_t i = 0; i < 96; ++i) if (i < a.hdr_syms) a.frame_out[i] = a.hdr[i];
        }
        if (tid < a.pad_bytes) a.frame_out[a.out_syms + tid] = 0;
        if constexpr (BCN) { if (tid < a.bcn_tail_len) a.frame_out[a.bcn_tail_off + tid] = (uint8_t)(a.bcn_tail_vals >> (8u * tid)); }   // after the last body byte
    }
}

// first lane group whose input a tile starting at stream symbol S needs (pixels: the packed converter starts at a
// multiple of 4 triples = 2 groups)
template <int FE>
__device__ __forceinline__ uint32_t first_group(uint32_t S) { return fe_px(FE) ? ((S / 13u) & ~3u) / 2u : ((S / 26u) & ~3u) / 2u; }   // (raw words: four word triples = two groups per lane)
// one past the last lane group: raw words stage whole lanes (four triples), so that no lane of the packed converter meets stale bytes
template <int FE>
__device__ __forceinline__ uint32_t end_group(uint32_t S) {
    constexpr uint32_t GS = fe_px(FE) ? kGroupSyms : kGroupSymsW;      // symbols per lane group
    return fe_px(FE) ? (S + GS - 1u) / GS : ((((S + 25u) / 26u) + 3u) & ~3u) / 2u;
}
// pipelined flow (input prefetch, packed converter): always in 1-D; in 2-D for pixel / RGB input (il_async != 0):
//   il_async == 1 (rows up to 512 symbols): the tile's input covers the whole row segments it overlaps; phase 1 leaves the symbols in
//     PRE-interleave order and a permutation pass by all waves moves them, in post-interleave order, into the stage buffer the
//     tile's input has just been consumed from (measured: cheaper than permuting in the three converting waves' stores);
//   il_async == 2 (wider rows): the tile's pre-interleave symbols are up to three runs (il_runs) staged one behind the other and
//     phase 1 stores every symbol at its post-interleave place -- no row is staged whole, any width.
// (Raw words in 2-D keep the row-by-row flow, phase1_sync_rows.)
// the runs of a tile and where each one's input sits in a stage buffer: run i at kRunPitch-rounded offsets (an LDS-DMA piece is
// a whole KiB, so a run's last piece may reach up to 1008 bytes past its end)
struct TileIn { uint32_t lo[3], hi[3], off[3], plo[3], n; };
template <int FE, int IL>
__device__ __forceinline__ TileIn tile_in(const EncArgs& a, uint32_t S, const uint32_t TS) {
    constexpr uint32_t GBf = FE == FE_PIXELS ? kGroupBytes : FE == FE_RGB ? kGroupBytesRgb : kGroupBytesW;
    TileIn T; T.n = 1; T.lo[0] = S; T.hi[0] = S + TS; T.off[0] = 0; T.lo[1] = T.lo[2] = T.hi[1] = T.hi[2] = 0; T.off[1] = T.off[2] = 0; T.plo[0] = S; T.plo[1] = T.plo[2] = 0;
    if constexpr (IL == 1 && fe_px(FE)) {                                  // narrow rows: the whole row segments the tile overlaps, one run
        if (S < a.n_sym) { T.lo[0] = enc_row(S, a).start; const IlRow gl = enc_row(min(S + TS, a.n_sym) - 1u, a); T.hi[0] = max(gl.start + gl.len, S + TS); }
        return T;
    }
    if constexpr (IL == 2 && fe_px(FE)) {
        const IlRuns R = il_runs(S, TS, a);
        T.n = R.n; uint32_t off = 0;
#pragma unroll
        for (uint32_t i = 0; i < 3; ++i) {
            T.lo[i] = R.lo[i]; T.hi[i] = R.hi[i]; T.off[i] = off; T.plo[i] = R.plo[i];
            const uint32_t bytes = (uint32_t)((uint64_t)end_group<FE>(R.hi[i]) * GBf - (((uint64_t)first_group<FE>(R.lo[i]) * GBf) & ~15ull));
            if (i < R.n) off += (bytes + 1023u + 16u) & ~1023u;
        }
    }
    return T;
}
template <int FE>
__device__ __forceinline__ void stage_tile(const EncArgs& a, const TileIn& T, uint32_t stage, uint32_t lane, uint32_t w, uint32_t nw, const uint64_t base = 0) {
#pragma unroll
    for (uint32_t i = 0; i < 3; ++i) if (i < T.n) stage_input<FE>(a, stage + T.off[i], first_group<FE>(T.lo[i]), end_group<FE>(T.hi[i]), lane, w, nw, base);
}

// A batch of equal frames in one launch (BATCH, enc_frames_k): the tile space is n_frames * a.n_tiles tickets.  Everything a tile derives
// from its index -- stream symbols, band offsets, scrambler phase, block counts, the ragged last tile -- comes from the tile's index
// inside its frame; only the frame's input and output base move.  One frame (the kernels above): the ticket is the tile, no offset; these
// helpers then stand for the plain expressions they replace.
// (fa: the batch's block, null for one frame.  encode_body keeps its `const EncArgs& a`: with the frame arguments reached through a
// second reference the 2-D run kernels, IL = 2, came out with other scalar spills.)
template <bool BATCH>
__device__ __forceinline__ uint32_t enc_n_tiles(const EncArgs& a, const EncFramesArgs* const fa) { if constexpr (BATCH) return fa->n_total; else return a.n_tiles; }
struct FrameTile { uint32_t tile, frame; };
template <bool BATCH>
__device__ __forceinline__ FrameTile frame_tile(const EncArgs& a, const EncFramesArgs* const fa, const uint32_t t) {
    FrameTile ft; ft.tile = t; ft.frame = 0;
    if constexpr (BATCH) { ft.frame = div_any(t, fa->div_tiles); ft.tile = t - ft.frame * a.n_tiles; }
    return ft;
}
// the frame's byte offset from a.in / from a.body_out
template <bool BATCH>
__device__ __forceinline__ uint64_t frame_in_off(const EncFramesArgs* const fa, const FrameTile& ft) { if constexpr (BATCH) return (uint64_t)ft.frame * fa->in_stride; else return 0; }
template <bool BATCH>
__device__ __forceinline__ uint64_t frame_out_off(const EncFramesArgs* const fa, const FrameTile& ft) { if constexpr (BATCH) return (uint64_t)ft.frame * fa->out_stride; else return 0; }
// header symbols and zero tail of every frame of a batch (write_frame_ends, one frame): workgroup w writes those of frames w, w + grid, ..
// in front of its first prefetch, so the stores are older than every input it waits for.  The header goes through LDS, a lane per byte:
// 96 stores by one thread inside the frame loop kept all 96 byte values in registers across it (24 VGPRs spilled).
__device__ __forceinline__ void write_batch_ends(const EncFramesArgs& fa, const uint32_t tid) {
    const EncArgs& a = fa.a;
    if (tid == 0) {                                                          // constant indices only (see above)
#pragma unroll
        for (uint32_t i = 0; i < 24; ++i) *(uint32_t*)(lds + kHdrFrames + 4u * i) = (uint32_t)a.hdr[4u * i] | (uint32_t)a.hdr[4u * i + 1u] << 8 | (uint32_t)a.hdr[4u * i + 2u] << 16 | (uint32_t)a.hdr[4u * i + 3u] << 24;
    }
    __syncthreads();
    for (uint32_t f = blockIdx.x; f < fa.n_frames; f += gridDim.x) {
        uint8_t* const fo = a.frame_out + (uint64_t)f * fa.out_stride;
        if (tid < a.hdr_syms) fo[tid] = (uint8_t)lds_u8(kHdrFrames + tid);
        if (tid < a.pad_bytes) fo[a.out_syms + tid] = 0;
    }
}

// Tiles are handed out dynamically: the three workgroups of a CU progress at different speeds (oldest wave first),
// up to 1.6x apart.  The first tile is blockIdx.x, every further one a ticket.  One counter serves ~11 ns per draw
// (memory-side atomic), too slow for 14k tiles, so workgroups and tiles are split into n_classes classes by index
// modulo n_classes, each with its own counter (class == XCD under round-robin dispatch, but nothing relies on it).
// a class's tiles are cls + NC j: j < wgc first tiles (= blockIdx), wgc <= j < 2 wgc second tiles (static too), then tickets
// the input of tile i+1 is requested at the top of tile i into the other stage buffer, by the waves that phase 1 (pixels)
// leaves idle: issuing the LDS-DMA costs ~400 cycles per KiB piece and would otherwise sit between the two phases
// Tickets are drawn by lane 0 of the LAST wave: the compiler turns the atomic into its wave-aggregated form, which reads the
// result back at once (s_waitcnt vmcnt(0): the atomic's round trip plus the acknowledgement of the wave's stores of the
// previous tile).  On thread 0 that stall sat in front of phase 1's conversion, on the critical path of every tile; the
// last wave has no conversion work (pixels), and is taken off prefetch duty so that the wait does not cover a DMA either.
// The roles rotate from tile to tile: a "virtual" wave index vw = wave - rot (mod nwv) decides who converts (vw < w0),
// who prefetches and who draws (vw = nwv - 1), and rot advances by w0 per tile.  Waves sit on SIMD (wave mod 4) for the
// whole kernel; with fixed roles the conversion -- more than half of the kernel's VALU work -- always ran on the same
// three SIMDs of a CU and those bounded the tile rate.  A ticket is drawn at the top of a tile and names the tile two after
// it (its input is requested at the top of the next tile): the drawing wave reads the atomic back at once anyway, so
// holding the ticket for one more tile only made the workgroups commit a tile earlier than needed (longer tail).
// (The decoders' Tickets, t3_decode_wg.h, are another protocol: drawn by wave 0, a slot per barrier parity, no static second round.)
struct EncTickets {
    bool dyn, excl;                  // tickets in use (pipelined flow, counters given); the drawing wave issues no prefetch
    uint32_t NC, cls, wgc;           // classes, this workgroup's, workgroups in this class
    uint32_t* ctr;                   // one counter per class, 256 B apart
    uint32_t w0, n_pf;               // waves that convert (planner: just enough lanes of four triples; raw words: two waves per lane unit); waves that prefetch
    uint32_t rot, par;               // role rotation; stage buffer parity
    template <int FE, bool FAST>
    __device__ __forceinline__ void setup(const EncArgs& a, const uint32_t nwv) {
        dyn = FAST && a.tile_ctr != nullptr;
        NC = a.n_classes; cls = blockIdx.x % NC;
        ctr = a.tile_ctr + 64u * cls;
        wgc = (gridDim.x - cls + NC - 1u) / NC;
        w0 = fe_px(FE) ? min(a.p1_wpp, nwv - 1u) : min(2u * min(a.p1_wpp, nwv / 2u), nwv - 1u);
        excl = dyn && w0 + 1u < nwv;
        n_pf = nwv - w0 - (excl ? 1u : 0u);
        par = 0; rot = 0;
    }
    __device__ __forceinline__ uint32_t second() const { return dyn ? cls + NC * (wgc + blockIdx.x / NC) : blockIdx.x + gridDim.x; }   // the static second tile
    __device__ __forceinline__ uint32_t vwave(const uint32_t wave, const uint32_t nwv) const { return wave >= rot ? wave - rot : wave + nwv - rot; }
    // the bare atomic into the slot, by lane 0 of the drawing wave: the tile after the next one (read() behind the symbol barrier)
    __device__ __forceinline__ void draw() const { *(uint32_t*)(lds + kHdrTicket) = cls + NC * (2u * wgc + atomicAdd(ctr, 1u)); }
    __device__ __forceinline__ uint32_t read() const { return __builtin_amdgcn_readfirstlane(*(const uint32_t*)(lds + kHdrTicket)); }
    __device__ __forceinline__ void advance(const uint32_t nwv) { par ^= 1u; rot = (rot + w0 >= nwv ? rot + w0 - nwv : rot + w0); }
    // done count, and re-arm for the next launch by whoever finishes last
    __device__ __forceinline__ void finish(const EncArgs& a, const uint32_t lane, const uint32_t wave, const uint32_t nwv) const {
        if (dyn && lane == 0u && wave == nwv - 1u) {                               // (not `tid`: it would stay live, or spilled, across the whole tile loop)
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                       // (every draw was read back by its wave right away)
            if (atomicAdd(a.tile_ctr + 64u * NC, 1u) == gridDim.x - 1u) {          // ... and so has everyone else's: re-arm for the next launch
                for (uint32_t c = 0; c <= NC; ++c) __hip_atomic_store(a.tile_ctr + 64u * c, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
};

// IL == 2, run-placed tiles: the odd rows' pieces inside the tile, reversed in place (dword pairs, bytes swapped): the tile's first row
// from S0, whole rows, the last row up to the tile's end -- one lane = the dwords i and n - 1 - i of a piece
__device__ __forceinline__ uint32_t reverse_rows_placed(const EncArgs& a, const uint32_t S0, const uint32_t TS, const uint32_t tid, const uint32_t nthr) {
    const uint32_t E = S0 + TS;
    const IlRow g0 = enc_row(S0, a); const uint32_t rl0 = g0.start, rn0 = g0.len, od0 = g0.odd;
    const uint32_t he = min(rl0 + rn0, E);                            // end of the first row's piece
    const uint32_t w8 = (a.il_w + 7u) >> 3;                           // lane tasks of a whole row
    const uint32_t n0 = od0 ? (he - S0 + 7u) >> 3 : 0u;
    const uint32_t rows = (E - he + a.il_w - 1u) / a.il_w;            // further rows the tile touches (the last one maybe in part)
    for (uint32_t t = tid; t < n0 + rows * w8; t += nthr) {
        uint32_t pa, len, i;                                          // piece start (post position), length, dword index
        if (t < n0) { pa = S0; len = he - S0; i = t; }
        else {
            const uint32_t ri = (t - n0) / w8; i = (t - n0) - ri * w8;
            pa = he + ri * a.il_w; len = min(a.il_w, E - pa);
            if (!enc_row(pa, a).odd) continue;
        }
        const uint32_t nd = len >> 2, j = nd - 1u - i;
        if (i > j || i >= nd) continue;
        const uint32_t ad = a.sym_off + (pa - S0);
        const uint32_t x = lds_u32(ad + 4u * i), y = lds_u32(ad + 4u * j);
        *T3_LDS(uint32_t, ad + 4u * i) = __builtin_bswap32(y);
        if (i != j) *T3_LDS(uint32_t, ad + 4u * j) = __builtin_bswap32(x);
    }
    barrier_lds();
    return a.sym_off;
}

// IL == 1, rows of whole 16-byte granules (round 3): the interleave maps every row of the chunk grid onto itself -- even rows stay,
// odd rows are mirrored -- and the symbol buffer holds whole rows (tile_in), so the odd rows are reversed IN PLACE: a lane swaps
// the 16-byte granules g and G - 1 - g of a row, bytes reversed; phase 2 then reads the tile at its offset inside the
// first row.  About a hundred lane tasks per tile; permute_rows (every symbol moved into the consumed stage buffer, two
// divisions per granule) took 3.5 k of a tile's 12 k cycles (stamp build, profiles/r03/notes.md).
__device__ __forceinline__ uint32_t reverse_rows16(const EncArgs& a, const uint32_t S0, const uint32_t u_lo, const uint32_t u_hi, const uint32_t tid, const uint32_t nthr) {
    const uint32_t G = a.il_w >> 4, G2 = (G + 1u) >> 1, n_rows = (u_hi - u_lo + a.il_w - 1u) / a.il_w;
    for (uint32_t t = tid; t < n_rows * G2; t += nthr) {
        const uint32_t ri = t / G2, g = t - ri * G2, p0 = u_lo + ri * a.il_w;
        if (p0 >= a.n_sym) continue;                                    // padding past the stream's end: identity
        // (left written out: enc_row forms the row's start before the parity test, one multiply earlier in the tile loop, not timed)
        const uint32_t chunk = div_ge2(p0, a.div_A), base = chunk * a.il_A, r = div_ge2(p0 - base, a.div_w);
        if (!(r & 1u)) continue;
        const uint32_t take = min(a.il_A, a.n_sym - base), rowlen = min(a.il_w, take - r * a.il_w);
        const uint32_t ra = a.sym_off + (p0 - u_lo);                    // 16-byte aligned: rows start at multiples of 16 from u_lo
        if (rowlen == a.il_w) {
            const uint32_t g1 = G - 1u - g;
            const u32x4 x = *T3_LDS(const u32x4, ra + 16u * g), y = *T3_LDS(const u32x4, ra + 16u * g1);
            *T3_LDS(u32x4, ra + 16u * g) = rev16(y);
            if (g1 != g) *T3_LDS(u32x4, ra + 16u * g1) = rev16(x);
        } else if (g == 0u) {                                           // the stream's last, short row: one lane, byte by byte
            for (uint32_t i = 0; 2u * i + 1u < rowlen; ++i) {
                const uint32_t lo = lds_u8(ra + i), hi = lds_u8(ra + rowlen - 1u - i);
                *T3_LDS(uint8_t, ra + i) = (uint8_t)hi; *T3_LDS(uint8_t, ra + rowlen - 1u - i) = (uint8_t)lo;
            }
        }
    }
    barrier_lds();
    return a.sym_off + (S0 - u_lo);
}

// IL == 1, other widths -- the permutation pass: post-interleave position v of the tile <- pre-interleave symbol il_perm(v) (an
// involution); one lane = 4 consecutive positions = one dword of the image phase 2 reads, in the stage buffer the tile's input came from.
// Rows of the chunk grid map onto themselves, and with rows that are multiples of 4 symbols (tile edges and chunk sizes
// are too) an aligned dword of a row stays an aligned dword: copied in even rows, byte-reversed from the mirrored
// column in odd rows.  Anything else (other widths, the stream's last short row, the padding past the stream's
// end) walks the cursor symbol by symbol.
__device__ __forceinline__ void permute_dword(const EncArgs& a, uint32_t v, const uint32_t S0, const uint32_t u_lo, const uint32_t stage, const bool rows4) {   // image dword at tile offset v - S0 (a multiple of 4)
    const uint32_t dst = stage + (v - S0);
    uint32_t w4 = 0;
    bool done = false;
    if (rows4 && v + 4u <= a.n_sym) {
        const IlRow rg = enc_row(v, a);
        if (!rg.odd) { w4 = lds_u32(a.sym_off + (v - u_lo)); done = true; }
        else if (rg.len == a.il_w) { w4 = __builtin_bswap32(lds_u32(a.sym_off + (rg.start + (a.il_w - 4u - (v - rg.start)) - u_lo))); done = true; }
    }
    if (!done) {
        IlCursor cur;
        if (v < a.n_sym) cur.init(v, a);
#pragma unroll
        for (uint32_t q = 0; q < 4; ++q, ++v) {
            uint32_t u = v;
            if (v < a.n_sym) { u = cur.get(); cur.next(a); }
            w4 |= lds_u8(a.sym_off + (u - u_lo)) << (8u * q);
        }
    }
    *T3_LDS(uint32_t, dst) = w4;
}
// (S0 .. stage by reference: by value the row predicates were hoisted apart and ORed inside the tile loop; permute_dword's rows4 by value:
// by reference the pass was unswitched on it)
__device__ __forceinline__ uint32_t permute_rows(const EncArgs& a, const uint32_t& S0, const uint32_t& TS, const uint32_t& u_lo, const uint32_t& stage, const uint32_t tid, const uint32_t nthr) {
    const bool rows4 = (a.il_w & 3u) == 0u && ((a.il_A & 3u) == 0u || a.il_A >= a.n_sym) && (S0 & 3u) == 0u;
    if (rows4 && (a.il_w & 15u) == 0u && ((a.il_A & 15u) == 0u || a.il_A >= a.n_sym)) {
        // rows are multiples of 16 symbols: one lane = one 16-byte granule of the stream (aligned in stream coordinates, so it
        // lies inside one row): one row computation per 16 symbols; the tile's ragged ends go dword by dword
        const uint32_t g0 = S0 & ~15u;
        for (uint32_t q = tid; g0 + 16u * q < S0 + TS; q += nthr) {
            const uint32_t v = g0 + 16u * q;
            if (v >= S0 && v + 16u <= S0 + TS && v + 16u <= a.n_sym) {
                const IlRow rg = enc_row(v, a);
                if (!rg.odd || rg.len == a.il_w) {
                    const uint32_t src = rg.odd ? rg.start + (a.il_w - 16u - (v - rg.start)) : v;
                    const u32x4 x = *T3_LDS(const u32x4, a.sym_off + (src - u_lo));           // 16-byte aligned: rows start at multiples of 16 from u_lo
                    const uint32_t dst = stage + (v - S0);                                  // only 4-byte aligned (tile edges are multiples of 4)
                    const u32x4 y = rg.odd ? rev16(x) : x;
                    *T3_LDS(u32x2a4, dst) = u32x2a4{y.x, y.y};
                    *T3_LDS(u32x2a4, dst + 8u) = u32x2a4{y.z, y.w};
                    continue;
                }
            }
            for (uint32_t d = 0; d < 4u; ++d) { const uint32_t vd = v + 4u * d; if (vd >= S0 && vd < S0 + TS) permute_dword(a, vd, S0, u_lo, stage, rows4); }
        }
    } else {
        for (uint32_t g = tid; 4u * g < TS; g += nthr) permute_dword(a, S0 + 4u * g, S0, u_lo, stage, rows4);
    }
    barrier_lds();
    return stage;
}

// Raw words in 2-D, the row-by-row flow (no prefetch, no tickets): the symbol buffer zeroed, and the lane groups [g_lo, g_hi) of the
// pre-interleave symbols this tile needs -- whole row segments.  The caller stages and converts them a stage buffer at a time
// (convert_groups stores every symbol at its post-interleave place)
template <int FE>
__device__ __forceinline__ void phase1_sync_rows(const EncArgs& a, const uint32_t& S0, const uint32_t& TS, const uint32_t& tid, const uint32_t& nthr, uint32_t& g_lo, uint32_t& g_hi) {
    constexpr uint32_t GS = fe_px(FE) ? kGroupSyms : kGroupSymsW;      // symbols per lane group
    __syncthreads();                                                  // everyone left phase 2 of the previous tile
    for (uint32_t i = tid * 16u; i < TS; i += nthr * 16u) *(uint4*)(lds + a.sym_off + i) = make_uint4(0, 0, 0, 0);
    uint32_t u_lo = S0, u_hi = S0;                                   // pre-interleave symbols this tile needs: whole row segments
    const uint32_t hi = min(S0 + TS, a.n_sym);
    if (S0 < hi) { u_lo = enc_row(S0, a).start; const IlRow gl = enc_row(hi - 1u, a); u_hi = gl.start + gl.len; }
    g_lo = u_lo / GS; g_hi = (u_hi + GS - 1u) / GS;
    __syncthreads();
}

// REGEO (recompute the block geometry per tile instead of keeping it across the tile loop, phase2_mfma): chosen per instantiation from the
// register allocator's result (profiles/kernel_resources.py: spilled VGPRs with / without) -- RS(26,20) from pixels / raw words
// fits the 80-VGPR budget as it is, most others stop spilling with it, a few spill less without it
constexpr bool enc_regeo(int FE, int IL, int RSEL, bool BCN) {
    return FE == FE_RGB ? (RSEL != 6 || IL == 2) : RSEL == 6 ? false
        : (FE == FE_PIXELS && IL == 0 && RSEL == 8 && !BCN) ? false
        : (FE == FE_PIXELS && IL == 2 && (RSEL == 2 || (RSEL == 4 && BCN))) ? false
        : (FE == FE_WORDS && IL == 1 && (RSEL == 2 || RSEL == 8)) ? false : true;
}
// ... of the batch kernels (enc_frames_k: the frame index and the strides ride along): RS(26,20) from pixels no longer fits as it is
constexpr bool enc_regeo_batch(int FE, int RSEL) { return enc_regeo(FE, 0, RSEL, false) || (FE == FE_PIXELS && RSEL == 6); }
// ... of the mixed-k kernel (LUT path): one lane = one block, dealt linearly across the bands.  A function of its own with its operands by
// reference: as a branch of phase2, which takes them by value, the address arithmetic of phase2_band's stores was scheduled differently
__device__ __forceinline__ void phase2_lut(const EncArgs& a, const uint32_t& symb, const uint32_t& tile, const uint32_t& tid) {
    if (tid < a.n_items) {
        const uint32_t item = tid;
        uint32_t b = 0;
#pragma unroll
        for (uint32_t q = 1; q < 9; ++q) if (item >= band_first(q)) b = q;
        const uint32_t m = item - band_first(b), nbt = band_row(b).nbt;
        switch (band_row(b).k) {                                         // lanes of one wave may sit in two bands (mixed k: divergent)
            case 24: phase2_band<2, false>(a, symb, tile, b, m, nbt); break;
            case 22: phase2_band<4, false>(a, symb, tile, b, m, nbt); break;
            case 20: phase2_band<6, false>(a, symb, tile, b, m, nbt); break;
            default: phase2_band<8, false>(a, symb, tile, b, m, nbt); break;
        }
    }
}
// Phase 2 of one tile: one lane = one RS block; a wave stays inside one band; stores go straight to HBM.  Returns the global store
// instructions this wave issued (`younger`, see barrier_input): single-k and UEP kernels count them (phase2_mfma); the mixed kernel
// does not (0 over-waits, which is safe).  Operands by value: by reference the single-k kernels reload scalars inside the tile loop
template <int FE, int IL, int RSEL, bool BCN, bool REGEO = enc_regeo(FE, IL, RSEL, BCN)>
__device__ __forceinline__ uint32_t phase2(const EncArgs& a, const uint32_t symb, const uint32_t tile, const uint32_t tid, const uint32_t lane, const uint32_t wave, const v4i (&Afr)[3], const uint64_t out_base = 0) {
    uint32_t younger = 0;
    if constexpr (RSEL > 1) {                                          // one k on all nine bands: both sets of the wave in one call
        P2Map M; M.item0[0] = wave * 64u; M.item0[1] = wave * 64u + 32u; M.n_items = a.n_items; M.nb = a.nb_uniform; M.div_nb = a.div_nb;
        M.band_tab = ~0u; M.scr_off = kHdrScr;
        younger = phase2_mfma<RSEL, false, BCN, REGEO>(a, symb, tile, lane, Afr, M, out_base);
    } else if constexpr (RSEL == 1) {                                  // UEP: a set lies inside one group of bands that share k
#pragma unroll
        for (uint32_t q = 0; q < 2; ++q) {
            const uint32_t set = wave + 8u * q;                         // sets go round the eight waves
            if (set >= a.n_sets) continue;
            const uint32_t st = __builtin_amdgcn_readfirstlane(*(const uint32_t*)(lds + kHdrSets + 4u * set));
            const uint32_t gb = kHdrGrp + kHdrGrpStride * (st & 0xFFu);
            P2Map M; M.item0[0] = st >> 8; M.item0[1] = 0xFFFF0000u;
            M.nb = __builtin_amdgcn_readfirstlane(*(const uint32_t*)(lds + gb)); M.div_nb.mul = __builtin_amdgcn_readfirstlane(*(const uint32_t*)(lds + gb + 4));
            M.div_nb.sh = __builtin_amdgcn_readfirstlane(*(const uint32_t*)(lds + gb + 8)); M.div_nb.d = __builtin_amdgcn_readfirstlane(*(const uint32_t*)(lds + gb + 12));
            M.n_items = __builtin_amdgcn_readfirstlane(*(const uint32_t*)(lds + gb + 16));
            const uint32_t rr = __builtin_amdgcn_readfirstlane(*(const uint32_t*)(lds + gb + 20)), ao = __builtin_amdgcn_readfirstlane(*(const uint32_t*)(lds + gb + 36));
            M.band_tab = gb + 24u; M.scr_off = gb + 48u;
            v4i Ag[3];
#pragma unroll
            for (int s = 0; s < 3; ++s) Ag[s] = *T3_LDS(const v4i, ao + 16u * (s * 64u + lane));
            switch (rr) {
                case 2: younger += phase2_mfma<2, true, BCN>(a, symb, tile, lane, Ag, M); break;
                case 4: younger += phase2_mfma<4, true, BCN>(a, symb, tile, lane, Ag, M); break;
                case 6: younger += phase2_mfma<6, true, BCN>(a, symb, tile, lane, Ag, M); break;
                default: younger += phase2_mfma<8, true, BCN>(a, symb, tile, lane, Ag, M); break;
            }
        }
    } else phase2_lut(a, symb, tile, tid);
    return younger;
}

// RSEL = 26-k when every band of the launch shares one k (the common case: no dead code paths, fewer registers,
// 640-thread bound so that two workgroups share a CU); RSEL = 0 handles mixed k with a wave-uniform switch.
// IL: 0 = 1-D; 1 = 2-D, whole rows + permutation pass (raw words: the row-by-row flow); 2 = 2-D, runs + permuting stores (wide rows)
// BATCH: fa is the batch's block (a = fa->a), the tile space that of all its frames (frame_tile); else fa is null
template <int FE, int IL, int RSEL, bool BCN, bool BATCH = false>
__device__ __forceinline__ void encode_body(const EncArgs& a, const EncFramesArgs* const fa = nullptr) {
    static_assert(!BATCH || (IL == 0 && !BCN && RSEL > 1 && fe_px(FE)), "batch launches: pixel / RGB input, one k, 1-D, no beacon");
    constexpr int SH = RSEL != 0 ? 2 : 3;                                     // symbol pre-scale: 4-byte T entries (MFMA) / 8-byte LUT entries
    constexpr bool fast = !IL || fe_px(FE);                                    // pipelined flow (the host sets a.il_async == IL for pixel / RGB input, 0 for raw words)
    const uint32_t tid = threadIdx.x, nthr = blockDim.x, lane = tid & 63u, wave = __builtin_amdgcn_readfirstlane(tid >> 6), nwv = nthr >> 6;
    const uint32_t TS = 9u * a.Lq;
    EncStamps st; st.enter();

    stage_enc_header<FE, RSEL>(a, tid, nthr);
    if constexpr (BATCH) write_batch_ends(*fa, tid); else write_frame_ends<BCN>(a, tid);

    v4i Afr[3] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};                   // single-k kernels: the parity matrix lives in 12 VGPRs
    if constexpr (RSEL > 1) {
#pragma unroll
        for (int s = 0; s < 3; ++s) Afr[s] = ((const v4i*)a.afrag)[s * 64 + lane];
        // Let these loads land here, with a wait the compiler's counter tracking sees (the builtin, not inline asm): otherwise it
        // protects their first use inside the tile loop with s_waitcnt vmcnt(0) in front of the first MFMA of every tile, which also
        // waits for the next tile's input prefetch and the previous tile's stores.
        __builtin_amdgcn_s_waitcnt(0x0F70);                                     // vmcnt(0) only (gfx9 encoding: vm[3:0] | exp << 4 | lgkm << 8 | vm[5:4] << 14)
    }
    st.arm();

    if constexpr (fast) {                                                    // prologue: first tile's input
        const FrameTile f0 = frame_tile<BATCH>(a, fa, blockIdx.x);
        if (blockIdx.x < enc_n_tiles<BATCH>(a, fa)) stage_tile<FE>(a, tile_in<FE, IL>(a, f0.tile * TS, TS), a.stage_off, lane, wave, nwv, frame_in_off<BATCH>(fa, f0));
    }
    uint32_t younger = 0;                                                    // VMEM ops this wave issued after its last prefetch
    EncTickets tk; tk.setup<FE, fast>(a, nwv);
    for (uint32_t tile = blockIdx.x, nxt = tk.second(), nn = 0; tile < enc_n_tiles<BATCH>(a, fa); tile = nxt, nxt = nn, tk.advance(nwv)) {
        const uint32_t vw = fast ? tk.vwave(wave, nwv) : wave;
        const bool drawer = tk.dyn && lane == 0u && vw == nwv - 1u;
        const FrameTile ft = frame_tile<BATCH>(a, fa, tile);                   // (one frame: the ticket itself)
        const uint32_t S0 = ft.tile * TS;
        const uint32_t stage = a.stage_off + (fast ? tk.par * a.stage_stride : 0u);
        uint32_t symb = a.sym_off;                                            // where phase 2 finds the tile's symbols
        // ---------------- phase 1: input -> stream-ordered symbols in LDS ----------------
        if constexpr (fast) {
            barrier_input(younger);                                           // this tile's input has landed, everyone left phase 2
            st.mark(0); st.landed();
            if (drawer) tk.draw();
#ifndef T3_ABL_NO_PREFETCH
            if (nxt < enc_n_tiles<BATCH>(a, fa) && vw >= tk.w0 && vw - tk.w0 < tk.n_pf) {   // (batch: the next tile may belong to another frame)
                const FrameTile fn = frame_tile<BATCH>(a, fa, nxt);
                stage_tile<FE>(a, tile_in<FE, IL>(a, fn.tile * TS, TS), a.stage_off + (tk.par ^ 1u) * a.stage_stride, lane, vw - tk.w0, tk.n_pf, frame_in_off<BATCH>(fa, fn));
            }
#endif
            st.mark(4);
            uint32_t u_lo = S0, u_hi = S0 + TS;
            bool placed = false;                                              // IL == 2: this tile goes through the run-placed flow
#ifndef T3_ABL_NO_P1
            if constexpr (fe_px(FE)) {
                const TileIn T = tile_in<FE, IL>(a, S0, TS);
                u_hi = T.hi[0];
                P1Run r0 = p1_run<FE>(T.lo[0], T.hi[0], stage + T.off[0]), r1 = p1_run<FE>(T.lo[1], T.hi[1], stage + T.off[1]), r2 = p1_run<FE>(T.lo[2], T.hi[2], stage + T.off[2]);
                if (T.n < 1u) r0.n_units = 0; if (T.n < 2u) r1.n_units = 0; if (T.n < 3u) r2.n_units = 0;
                u_lo = T.lo[0];
                if constexpr (IL == 2) {
                    // run-placed flow (round 3): whole rows of multiples of 4 symbols, the tile inside the stream; the stream's last tiles
                    // (ragged last row, padding) and other geometries keep the cursor flow
                    placed = (a.il_w & 3u) == 0u && ((a.il_A & 3u) == 0u || a.il_A >= a.n_sym) && (S0 & 3u) == 0u && (TS & 3u) == 0u && S0 + TS <= a.n_sym
                             && enc_row(S0 + TS - 1u, a).len == a.il_w;
                    r0.dst0 = a.sym_off + (T.plo[0] - S0) - T.lo[0]; r1.dst0 = a.sym_off + (T.plo[1] - S0) - T.lo[1]; r2.dst0 = a.sym_off + (T.plo[2] - S0) - T.lo[2];   // (wraps; dst0 + u does not)
                }
                if constexpr (IL == 1) convert_pixels_packed<(1 << SH), FE, false>(a, r0, r1, r2, u_lo, TS, lane, vw, nwv);   // pre-interleave order; the pass below moves them
                else convert_pixels_packed<(1 << SH), FE, IL == 2>(a, r0, r1, r2, S0, TS, lane, vw, nwv, placed);
            } else convert_words_packed<SH>(a, w1_run(S0, S0 + TS, stage), S0, lane, vw, nwv);
#endif
            st.mark(5);                                                       // (diagnostic) this wave's conversion
            barrier_lds();                                                    // symbols complete
            st.mark(1);
            nn = tk.dyn ? tk.read() : nxt + gridDim.x;                        // the tile after the next one
            if (IL == 2 && placed) symb = reverse_rows_placed(a, S0, TS, tid, nthr);
            if (IL == 1 && (a.il_w & 15u) == 0u) { symb = reverse_rows16(a, S0, u_lo, u_hi, tid, nthr); st.mark(3); }
            else if constexpr (IL == 1) { symb = permute_rows(a, S0, TS, u_lo, stage, tid, nthr); st.mark(3); }
        } else {
            nn = nxt + gridDim.x;
            uint32_t g_lo, g_hi;
            phase1_sync_rows<FE>(a, S0, TS, tid, nthr, g_lo, g_hi);
            // (the chunk loop stays written out: inside a function every raw-word 2-D kernel's tile loop came out with other branches, not timed)
            for (uint32_t gc = g_lo; gc < g_hi; gc += a.stage_groups) {
                const uint32_t gc_hi = min(g_hi, gc + a.stage_groups);
                stage_input<FE>(a, stage, gc, gc_hi, lane, wave, nwv);
                __syncthreads();
                st.mark(0);
                convert_groups<FE, true, SH>(a, stage, gc, gc, gc_hi, S0, TS, tid, nthr);
                __syncthreads();
                st.mark(1);
            }
        }

        // ---------------- phase 2 ----------------
        younger = 0;
#ifndef T3_ABL_NO_P2
        if constexpr (BATCH) younger = phase2<FE, IL, RSEL, BCN, enc_regeo_batch(FE, RSEL)>(a, symb, ft.tile, tid, lane, wave, Afr, frame_out_off<BATCH>(fa, ft));
        else younger = phase2<FE, IL, RSEL, BCN>(a, symb, tile, tid, lane, wave, Afr);
#endif
        st.mark(2);
    }
    tk.finish(a, lane, wave, nwv);
    st.report(a, tid);
}

constexpr int kEncWavesPerEu = 6;   // <= 80 VGPRs: three 8-wave workgroups per CU
template <int FE, int IL, int RSEL, bool BCN>
__global__ __launch_bounds__(512, kEncWavesPerEu) void encode_kernel_k(const EncArgs a) { encode_body<FE, IL, RSEL, BCN>(a); }
template <int FE, int IL, bool BCN>
__global__ __launch_bounds__(512, kEncWavesPerEu) void encode_kernel_uep(const EncArgs a) { encode_body<FE, IL, 1, BCN>(a); }   // UEP on the matrix cores
template <int FE, int IL>
__global__ __launch_bounds__(1024) void encode_kernel_mixed(const EncArgs a) { encode_body<FE, IL, 0, false>(a); }

#define T3_INST_KB(FE, IL, BCN) \
    template __global__ void encode_kernel_k<FE, IL, 2, BCN>(const EncArgs); template __global__ void encode_kernel_k<FE, IL, 4, BCN>(const EncArgs); \
    template __global__ void encode_kernel_k<FE, IL, 6, BCN>(const EncArgs); template __global__ void encode_kernel_k<FE, IL, 8, BCN>(const EncArgs); \
    template __global__ void encode_kernel_uep<FE, IL, BCN>(const EncArgs);
#define T3_INST_K(FE, IL) T3_INST_KB(FE, IL, false) T3_INST_KB(FE, IL, true) template __global__ void encode_kernel_mixed<FE, IL>(const EncArgs);

// a batch of equal frames (t3_encode_frames.hip): pixels / RGB in, one k = 26 - R on all bands, 1-D, no beacon
template <int FE, int R>
__global__ __launch_bounds__(512, kEncWavesPerEu) void enc_frames_k(const EncFramesArgs fa) { encode_body<FE, 0, R, false, true>(fa.a, &fa); }

}  // namespace t3
