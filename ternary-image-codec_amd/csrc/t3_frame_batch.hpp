// t3_frame_batch.hpp — what the synchronous repair and erasure-decode entries (t3_api_repair.cpp, t3_api_decode_era.cpp) decide on the host
// about one frame and about a batch of equal frames, each rule once: which header counts, which frames run together, which addresses a
// batch may have, how the host entries stage it, what the fetched verdict words become.  Pure C++17, no device (tests/test_frame_batch.py).
#pragma once
#include "t3_decode.h"
#include "t3_host.hpp"

namespace t3 {

// One frame's header as the synchronous entries see it.  ok: it decodes (RS + CRC-12) and counts (accept_header)
struct FrameHeader { bool ok; t3_cfg cfg; uint64_t n_raw; uint8_t next[3]; };

// The 90 header bytes `got` of a frame of n_in words, parsed over the caller's `seen`.  The header counts only if plan_of(n_raw, cfg, L) -- the
// entry's planner, and what else it checks in front of the truncation -- gives T3_OK and the n_in words hold the framing L.
// T3_OK (h.ok), T3_E_HEADER (no header, or a truncated stream), else plan_of's code as it is.
template <class PlanFn> int accept_header(const uint8_t got[90], uint64_t n_in, const t3_cfg& seen, FrameHeader& h, t3_layout& L, PlanFn plan_of) {
    h.ok = false; h.cfg = seen; h.n_raw = 0;
    if (header_parse(got, n_in, T3_MODE_FIXED, h.cfg, &h.n_raw, h.next) != T3_OK) return T3_E_HEADER;
    { const int rc = plan_of(h.n_raw, h.cfg, L); if (rc) return rc; }
    h.ok = L.out_words <= n_in;
    return h.ok ? T3_OK : T3_E_HEADER;
}
// Every header of a batch (got: 90 bytes a frame, back to back) by plan_of(f, n_raw, cfg, L): hd[f], L[f], go[f] = hd[f].ok -- a frame whose
// plan fails is simply not ok.  *seen becomes the configuration of the first header that counts (OLD:1006-1013); false: none does.
template <class PlanFn> bool parse_headers(const uint8_t* got, uint32_t n_frames, uint64_t n_in, t3_cfg* seen, FrameHeader* hd, t3_layout* L, uint8_t* go, PlanFn plan_of) {
    bool any = false;
    for (uint32_t f = 0; f < n_frames; ++f) {
        accept_header(got + 90ull * f, n_in, *seen, hd[f], L[f], [&](uint64_t n_raw, const t3_cfg& cfg, t3_layout& l) { return plan_of(f, n_raw, cfg, l); });
        go[f] = hd[f].ok ? 1 : 0;
        if (hd[f].ok && !any) { any = true; *seen = hd[f].cfg; }
    }
    return any;
}

// The bytes a header that decodes is rewritten to (repair): its own three RS(26,18) codewords and 12 zero symbols, which are
// what t3hip_header_encode gives for the frame's configuration; the parsed configuration does not carry every field those come from (the
// scrambler travels as its next-state table).  *differs: from `got`.  false: a block does not decode
bool header_codewords(const uint8_t got[90], uint8_t fix[90], uint8_t* differs);

// The next maximal run [*f0, *f1) of consecutive go frames of one configuration, one n_raw_words and one scrambler table (hd null: of
// go frames, whatever they hold) at or behind `from`: one batched body, or one copy, each.  false: no go frame is left
bool next_run(const uint8_t* go, const FrameHeader* hd, uint32_t n_frames, uint32_t from, uint32_t* f0, uint32_t* f1);

// The coded frames of a batch on the device: an even base, n_in words whose bytes 64 bits count, and (two frames or more; one: the stride
// is not looked at) an even stride apart without overlap
inline bool batch_in_ok(const void* base, uint64_t n_in, uint64_t stride, uint32_t n_frames) {
    return ((uintptr_t)base & 1u) == 0 && n_in <= (~0ull) / 9 && (n_frames < 2 || ((stride & 1u) == 0 && stride >= 9 * n_in));
}
// How a host entry stages coded frames lying `stride` apart: only a frame's `bytes` travel, on the device the frames lie an even
// `dev_stride` of their own apart, and `pitch` is the caller's (one frame: the stride is not looked at)
struct FrameStage { uint64_t bytes, dev_stride, pitch; };
inline FrameStage frame_stage(uint64_t n_in, uint64_t stride, uint32_t n_frames) { const uint64_t fb = 9 * n_in; return FrameStage{fb, fb + (fb & 1u), n_frames > 1 ? stride : fb}; }

// A frame whose configuration the caller names: the header symbols it encodes to (hs of them) and the scrambler's next-state table
struct KnownFrame { HdrExpect hx; uint32_t hs; uint8_t next[3]; };
KnownFrame known_frame(const t3_cfg& cfg, uint64_t n_raw);

// The frames a batch decode runs; go[f] in: the header counts.  The first of them fixes the batch's units (returned); a frame of another
// units_of[f] is not of this batch (go cleared, its code stays); units > cap_units: T3_E_CAPACITY for every frame of the batch, none runs
uint64_t select_equal_frames(const uint64_t* units_of, uint32_t n_frames, uint64_t cap_units, uint8_t* go, int* frame_rc);

// The fetched verdict words v (nw a frame) of the frames that ran (go; null: all): counts[nw f + 1 ..] = the words, frame_rc[f] = T3_E_RS when
// word 1 says so, else T3_OK.  A frame that did not run keeps counts and code: its words were never written
void fold_verdicts(const uint32_t* v, uint32_t nw, uint32_t n_frames, const uint8_t* go, uint32_t* counts, int* frame_rc);

}  // namespace t3
