// t3_frame_batch.cpp — the host-side rules of the synchronous repair and erasure-decode entries over one frame and over a batch of equal
// frames (t3_frame_batch.hpp).  No device.
#include "t3_frame_batch.hpp"

#include <string.h>

namespace t3 {

bool header_codewords(const uint8_t got[90], uint8_t fix[90], uint8_t* differs) {
    for (int q = 0; q < 3; ++q) {
        for (int i = 0; i < 26; ++i) fix[26 * q + i] = got[26 * q + i] % 27;
        if (!rs_decode_host(18, fix + 26 * q, true)) return false;                 // (header_parse has accepted them)
    }
    memset(fix + 78, 0, 12);
    *differs = memcmp(got, fix, 90) != 0 ? 1 : 0;
    return true;
}

static bool same_run(const FrameHeader& a, const FrameHeader& b) {
    return a.n_raw == b.n_raw && memcmp(&a.cfg, &b.cfg, sizeof(t3_cfg)) == 0 && memcmp(a.next, b.next, 3) == 0;
}
bool next_run(const uint8_t* go, const FrameHeader* hd, uint32_t n_frames, uint32_t from, uint32_t* f0, uint32_t* f1) {
    while (from < n_frames && !go[from]) ++from;
    if (from >= n_frames) return false;
    uint32_t end = from + 1;
    while (end < n_frames && go[end] && (!hd || same_run(hd[end], hd[from]))) ++end;
    *f0 = from; *f1 = end;
    return true;
}

KnownFrame known_frame(const t3_cfg& cfg, uint64_t n_raw) {
    KnownFrame k; memset(&k, 0, sizeof k);
    k.hs = (uint32_t)header_encode(cfg, n_raw, k.hx.b);
    memcpy(k.next, scrambler_cycle(cfg.seed_a, cfg.seed_b, cfg.seed_s0).next, 3);
    return k;
}

uint64_t select_equal_frames(const uint64_t* units_of, uint32_t n_frames, uint64_t cap_units, uint8_t* go, int* frame_rc) {
    bool any = false; uint64_t units = 0;
    for (uint32_t f = 0; f < n_frames; ++f) {
        if (!go[f]) continue;
        if (!any) { any = true; units = units_of[f]; }
        if (units_of[f] != units) go[f] = 0;                                       // T3_E_HEADER
        else if (units > cap_units) { go[f] = 0; frame_rc[f] = T3_E_CAPACITY; }
    }
    return units;
}

void fold_verdicts(const uint32_t* v, uint32_t nw, uint32_t n_frames, const uint8_t* go, uint32_t* counts, int* frame_rc) {
    for (uint32_t f = 0; f < n_frames; ++f) {
        if (go && !go[f]) continue;
        for (uint32_t i = 1; i < nw; ++i) counts[nw * f + i] = v[nw * f + i];
        frame_rc[f] = v[nw * f + 1] ? T3_E_RS : T3_OK;
    }
}

}  // namespace t3
