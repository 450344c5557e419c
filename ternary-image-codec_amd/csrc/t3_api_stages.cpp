// t3_api_stages.cpp — C-ABI of the reference decoder's frame-sized stages taken one at a time (t3_decode_stages.hip):
//   descramble_words_inplace           OLD:938-947  -> t3hip_descramble_words[_dev]
//   demap_and_rsdecode_bands_from_words OLD:948-993 -> t3hip_demap_rsdecode_bands[_dev] (+ _syms: the output size)
// Stage 1 (read_and_decode_header_from_words OLD:918-937) is control data: host code in include/ternary_codec_v6.hpp.
#include <hip/hip_runtime.h>
#include <string.h>

#include <mutex>

#include "../../include/t3hip.h"
#include "t3_ctx.hpp"
#include "t3_decode.h"

using namespace t3;

namespace {
// Band geometry of OLD:950-991 for a body of n_words words: band b = slot b of every word, minus the beacon words of the beacon slot;
// band b uses code band_profile[b] % 4.  False when a code a band uses is not RS(26, 18 | 20 | 22 | 24) in arithmetic 0 / 1.
struct StagePlan { uint32_t k[9], fixed[9]; uint64_t blocks[9], off[9], total; uint32_t bcn_band; uint32_t period; };
bool plan_stages(uint64_t n_words, const t3_cfg& h, const uint8_t code_k[4], const uint8_t* code_mode, StagePlan& P) {
    memset(&P, 0, sizeof P);
    const bool skip = h.beacon_enabled && h.beacon_words_period > 0;           // OLD:952
    P.bcn_band = skip && h.beacon_band_slot < 9 ? h.beacon_band_slot : 9u;       // a slot >= 9 never matches
    P.period = h.beacon_words_period;
    for (int b = 0; b < 9; ++b) {
        const int code = h.band_profile[b] % 4;
        if (!valid_k(code_k[code]) || (code_mode && code_mode[code] > 1)) return false;
        P.k[b] = code_k[code]; P.fixed[b] = code_mode ? code_mode[code] : 0;
        const uint64_t syms = (uint32_t)b == P.bcn_band ? n_words - (n_words + P.period - 1) / P.period : n_words;
        P.blocks[b] = syms / 26;                                                 // whole blocks only (OLD:983)
        P.off[b] = P.total; P.total += P.blocks[b] * P.k[b];
    }
    return true;
}
}  // namespace

extern "C" {

// ---- stage 2: descramble_words_inplace (OLD:938-947) ----
int t3hip_descramble_words_dev(void* d_words, uint64_t n_words, uint32_t a, uint32_t b, uint32_t s0, void* stream) {
    if (!ctx().ready) return T3_E_NODEVICE;
    if (!n_words) return T3_OK;
    if (!d_words) return T3_E_ARG;
    const ScrCycle sc = scrambler_cycle(a, b, s0);
    DescrArgs d; d.words = (uint8_t*)d_words; d.n_bytes = 9 * n_words; d.cyc24 = sc.cyc24; d.pre0 = sc.pre[0]; d.pre1 = sc.pre[1];
    hipLaunchKernelGGL(descramble_words_kernel, dim3(blocks_for((d.n_bytes + 63) / 64, 256u * 8u)), dim3(256), 0, (hipStream_t)stream, d);
    HIPCHK(hipGetLastError()); return T3_OK;
}
int t3hip_descramble_words(void* words9, uint64_t n_words, uint32_t a, uint32_t b, uint32_t s0) {
    Ctx& c = ctx(); if (!c.ready) return T3_E_NODEVICE;
    std::lock_guard<std::recursive_mutex> hl(c.host_mu);
    if (!n_words) return T3_OK;
    if (!words9) return T3_E_ARG;
    void *di, *dout; int rc = host_stage(c, words9, 9 * n_words, &di, 0, &dout); if (rc) return rc;
    rc = t3hip_descramble_words_dev(di, n_words, a, b, s0, c.stream); if (rc) return rc;
    return host_fetch(c, words9, di, 9 * n_words);
}

// ---- stage 3: demap_and_rsdecode_bands_from_words (OLD:948-993) ----
uint64_t t3hip_demap_rsdecode_bands_syms(uint64_t n_words, const t3_cfg* hdr, const uint8_t code_k[4]) {
    StagePlan P;
    if (!hdr || !code_k || !plan_stages(n_words, *hdr, code_k, nullptr, P)) return 0;
    return P.total;
}
int t3hip_demap_rsdecode_bands_dev(const void* d_body, uint64_t n_words, const t3_cfg* hdr, const uint8_t code_k[4], const uint8_t code_mode[4],
                                   uint8_t* d_out, uint64_t cap, uint64_t* d_n_valid, void* stream) {
    Ctx& c = ctx(); if (!c.ready) return T3_E_NODEVICE;
    StagePlan P;
    if (!hdr || !code_k || !code_mode || !d_n_valid || !plan_stages(n_words, *hdr, code_k, code_mode, P)) return T3_E_ARG;
    if (P.total > cap) return T3_E_CAPACITY;
    if (P.total && (!d_body || !d_out)) return T3_E_ARG;
    if (((uintptr_t)d_n_valid & 7u) != 0) return T3_E_ARG;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(fill_u64_kernel, dim3(1), dim3(1), 0, s, d_n_valid, P.total);
    HIPCHK(hipGetLastError());
    if (!P.total) return T3_OK;
    StageDecArgs a; memset(&a, 0, sizeof a);
    a.body = (const uint8_t*)d_body; a.out = d_out; a.n_valid = d_n_valid; a.tab = c.d_tab;
    for (int b = 0; b < 9; ++b) { a.band_k[b] = P.k[b]; a.band_fixed[b] = P.fixed[b]; a.band_off[b] = P.off[b]; }
    a.nb = n_words / 26; a.bcn_band = P.bcn_band;
    a.bcn_blocks = P.bcn_band < 9 ? P.blocks[P.bcn_band] : 0;
    a.div_p1 = to_dev(fastdiv(P.bcn_band < 9 && P.period > 1 ? P.period - 1 : 1));
    const uint64_t grid = (a.nb + kStageBlocks - 1) / kStageBlocks;        // every band has at most nb blocks
    if (grid > 0x7FFFFFFFull) return T3_E_ARG;
    hipLaunchKernelGGL(stage_decode_kernel, dim3((unsigned)grid), dim3(kStageThreads), 0, s, a);
    HIPCHK(hipGetLastError()); return T3_OK;
}
int t3hip_demap_rsdecode_bands(const void* body9, uint64_t n_words, const t3_cfg* hdr, const uint8_t code_k[4], const uint8_t code_mode[4],
                               uint8_t* out, uint64_t cap, uint64_t* n_out) {
    Ctx& c = ctx(); if (!c.ready) return T3_E_NODEVICE;
    std::lock_guard<std::recursive_mutex> hl(c.host_mu);
    StagePlan P;
    if (!n_out || !hdr || !code_k || !code_mode || !plan_stages(n_words, *hdr, code_k, code_mode, P)) return T3_E_ARG;
    *n_out = P.total;
    if (P.total > cap) return T3_E_CAPACITY;
    if ((n_words && !body9) || (P.total && !out)) return T3_E_ARG;
    const uint64_t nv_off = (P.total + 7) & ~7ull;                          // the prefix length behind the symbols, 8-byte aligned
    void *di, *dout; int rc = host_stage(c, body9, 9 * n_words, &di, nv_off + 8, &dout); if (rc) return rc;
    uint64_t* d_nv = (uint64_t*)((uint8_t*)dout + nv_off);
    rc = t3hip_demap_rsdecode_bands_dev(di, n_words, hdr, code_k, code_mode, (uint8_t*)dout, P.total, d_nv, c.stream); if (rc) return rc;
    uint64_t nv = 0;
    HIPCHK(hipMemcpyAsync(&nv, d_nv, 8, hipMemcpyDeviceToHost, c.stream));
    rc = host_fetch(c, out, dout, P.total); if (rc) return rc;
    *n_out = nv;
    return nv == P.total ? T3_OK : T3_E_RS;                                  // OLD:987: false, out_syms = the blocks in front of the failing one
}

}  // extern "C"
