// t3_api_record.cpp — the frame index record and CRC-32 part of the C-ABI (include/t3hip.h): the operator algebra behind the device
// tables, the tables themselves (crc_init), plan_crc / launch_crc, their forms for N equal streams (plan_crc_frames /
// launch_crc_frames) and the entry points.  Kernels: t3_crc_fp4.hip, t3_decode.hip, t3_crc_frames.hip.
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <vector>

#include "../../include/t3hip.h"
#include "t3_crc.h"
#include "t3_ctx.hpp"

using namespace t3;

namespace {
// A GF(2)-linear map on the 32-bit CRC register: col[b] = the image of register bit b.  Every operator here is a power of the
// generator, so they commute.
struct CrcOp {
    uint32_t col[32];
    uint32_t apply(uint32_t v) const { uint32_t r = 0; for (int b = 0; b < 32; ++b) if (v >> b & 1u) r ^= col[b]; return r; }
    static CrcOp compose(const CrcOp& a, const CrcOp& b) { CrcOp r; for (int i = 0; i < 32; ++i) r.col[i] = a.apply(b.col[i]); return r; }   // a after b
    static CrcOp identity() { CrcOp r; for (int b = 0; b < 32; ++b) r.col[b] = 1u << b; return r; }
    static CrcOp zero_byte() {                                        // the generator: one zero byte through the bitwise register update
        CrcOp r;
        for (int b = 0; b < 32; ++b) { uint32_t v = 1u << b; for (int i = 0; i < 8; ++i) v = (v & 1u) ? (0xEDB88320u ^ (v >> 1)) : (v >> 1); r.col[b] = v; }
        return r;
    }
    static CrcOp append_zero_bytes(uint64_t n) {                      // square-and-multiply (bitwise, 8 n steps would be too slow)
        CrcOp acc = identity(), op = zero_byte();
        for (; n; n >>= 1) { if (n & 1u) acc = compose(op, acc); op = compose(op, op); }
        return acc;
    }
};

// the CRC's leading 0xFFFFFFFF carried through n zero bytes
uint32_t crc_lead(uint64_t n_bytes) {
    static thread_local uint64_t last_n = ~0ull; static thread_local uint32_t last_x = 0;   // (a stream of frames of one size asks the same question every frame)
    if (n_bytes != last_n) { last_x = CrcOp::append_zero_bytes(n_bytes).apply(0xFFFFFFFFu); last_n = n_bytes; }
    return last_x;
}

// FP4 CRC with strided rounds (t3_crc_fp4.hip): wave g owns rounds g, g + W, ...; a column's running remainder re-enters 2048 W bytes
// further on.  W = every wave slot of the chip -- four-wave workgroups, two waves per SIMD: a wave needs ~100 VGPRs (the bit matrix),
// which is what a SIMD has left beside the decoder's six waves, so the kernel can start under the decode instead of behind it (16-wave
// workgroups had to wait for the decoder's persistent workgroups to drain: +0.1 ms per step) -- halved per level for shorter streams.
constexpr int kCrcStrideLevels = 8;
uint32_t crc_slots(const Ctx& c) { return (uint32_t)c.n_cu * 4u * 2u; }
uint32_t crc_stride_w(uint32_t slots, int l) { return std::max(4u, (slots >> l) & ~3u); }

// One [64][4] slice of the FP4 kernel's A operand for an operator on the running remainder: K slot 8 g + q (g, q < 4) of lane half kh
// carries the remainder bit of accumulator e = 4 g + q, row (e & 3) + 8 (e >> 2) + 4 kh, as FP4 0.5 (weight 2.0); the other slots are
// unused.  Lane l = m + 32 kh holds row m (t3_host.cpp build_mfma_encode).  FP4 e2m1: 0b0001 = 0.5, 0b0010 = 1.0, 0b0100 = 2.0.
void remainder_slice(const CrcOp& op, uint32_t* slice) {
    for (int kh = 0; kh < 2; ++kh) for (int e = 0; e < 16; ++e) {
        const uint32_t vec = op.col[(e & 3) + 8 * (e >> 2) + 4 * kh];
        for (int m = 0; m < 32; ++m) if (vec >> m & 1u) slice[(size_t)(m + 32 * kh) * 4 + (e >> 2)] |= 4u << (4 * (e & 3));
    }
}

int upload(uint32_t*& d, const std::vector<uint32_t>& h) {
    HIPCHK(hipMalloc((void**)&d, h.size() * 4));
    HIPCHK(hipMemcpy(d, h.data(), h.size() * 4, hipMemcpyHostToDevice));
    return T3_OK;
}

// The three test / measurement knobs, read on every call (the tests set them in a process whose library is loaded)
struct CrcKnobs { bool tables, blocked, atomics; };
CrcKnobs crc_knobs() {
    return {getenv("T3HIP_CRC_TABLES") != nullptr,                   // the table kernel for every stream
            getenv("T3HIP_CRC_BLOCKED") != nullptr,                  // round-2 assignment (consecutive rounds per wave)
            getenv("T3HIP_CRC_ATOMICS") != nullptr};                 // accumulators + atomics although the caller has room for partials
}

// CRC + symbol-sum accumulation of a payload, as decided by plan_crc and issued by launch_crc.  The matrix-core kernel takes whole
// streams (its first workgroup the rest behind the last 2 KiB round); crc_chunks_kernel takes every stream it does not.
enum class CrcForm { Tables, Fp4Blocked, Fp4Strided };
struct CrcPlan {
    CrcForm form;
    CrcMArgs m; uint32_t m_grid;                                     // crc_fp4_kernel (form != Tables)
    CrcArgs t; uint32_t t_grid;                                      // crc_chunks_kernel (form == Tables; 0: an empty stream, no launch)
    uint32_t* acc;                                                   // acc[0] xor, acc[1] symbol sum
    uint32_t n_partials;                                             // the workgroups store this many (xor, sum) side by side; 0 = accumulators + atomics
    bool zero_acc;                                                   // exactly when no partials are written
};

// partials / cap_wg (frame record; nullptr / 0: none): when the strided FP4 kernel runs and its grid fits cap_wg, the workgroups store
// their contributions in `partials` and the accumulators are left alone: no 8-byte fill kernel in front (4.5 us of stream time) and no
// atomics; the record kernel folds them.
CrcPlan plan_crc(const Ctx& c, const uint8_t* d_data, uint64_t n_bytes, uint32_t* acc, uint32_t* partials, uint32_t cap_wg) {
    const CrcKnobs knob = crc_knobs();
    CrcPlan p; memset(&p, 0, sizeof p); p.acc = acc;
    const bool mfma = ((uintptr_t)d_data & 15u) == 0 && n_bytes >= 64 * 2048 && (n_bytes >> 11) < (1ull << 32) && n_bytes < (1ull << kCrcPows) && !knob.tables;   // (the blocked form's epilogue walks the distance bit by bit over kCrcPows operators)
    if (mfma) {
        CrcMArgs& m = p.m;
        m.data = d_data; m.n_bytes = n_bytes; m.n_rounds = (uint32_t)(n_bytes >> 11);
        const uint32_t slots = crc_slots(c);
        m.rounds_per_wave = (uint32_t)std::max<uint64_t>(8, ((uint64_t)m.n_rounds + slots - 1) / slots);   // at least 8 rounds per wave
        m.afrag = c.crc.afrag4; m.zpow = c.crc.zpow; m.chunk_crc = acc; m.sym_sum = acc + 1;
        m.tail_len = (uint32_t)(n_bytes - ((uint64_t)m.n_rounds << 11));   // one more workgroup, first in the grid, takes the rest
        const uint32_t tail_wg = m.tail_len ? 1u : 0u;
        if (knob.blocked) {
            const uint64_t waves = ((uint64_t)m.n_rounds + m.rounds_per_wave - 1) / m.rounds_per_wave;
            p.form = CrcForm::Fp4Blocked; p.m_grid = (uint32_t)((waves + 3) / 4 + tail_wg);
        } else {
            int l = 0;                                                // halve W until a wave has at least 8 rounds
            while (l + 1 < kCrcStrideLevels && (uint64_t)crc_stride_w(slots, l) * 8 > m.n_rounds) ++l;
            m.stride_waves = crc_stride_w(slots, l); m.afb = c.crc.afb + (size_t)l * 64 * 4;
            m.dist_lo = c.crc.dist_lo; m.dist_hi = c.crc.dist_hi; m.last_mod = (m.n_rounds - 1u) % m.stride_waves;
            p.form = CrcForm::Fp4Strided; p.m_grid = m.stride_waves / 4 + tail_wg;
            if (partials && !knob.atomics && p.m_grid <= std::min(cap_wg, kRecordPartialWgs)) { m.partials = partials; p.n_partials = p.m_grid; }
        }
    } else {
        p.form = CrcForm::Tables;
        CrcArgs& t = p.t;
        t.data = d_data; t.n_bytes = n_bytes; t.chunk_bytes = 2304;   // 256 words per lane
        t.n_chunks = (uint32_t)((n_bytes + t.chunk_bytes - 1) / t.chunk_bytes);
        t.chunk_crc = acc; t.sym_sum = acc + 1; t.zpow = c.crc.zpow;
        p.t_grid = (t.n_chunks + 255) / 256;
    }
    p.zero_acc = p.n_partials == 0;
    return p;
}

int launch_crc(const CrcPlan& p, hipStream_t s) {
    if (p.zero_acc) HIPCHK(hipMemsetAsync(p.acc, 0, 8, s));
    if (p.form != CrcForm::Tables) { hipLaunchKernelGGL(crc_fp4_kernel, dim3(p.m_grid), dim3(256), 0, s, p.m); HIPCHK(hipGetLastError()); }
    else if (p.t_grid) { hipLaunchKernelGGL(crc_chunks_kernel, dim3(p.t_grid), dim3(256), 0, s, p.t); HIPCHK(hipGetLastError()); }
    return T3_OK;
}

// CRC-32 of a device buffer, on s and waited for: one accumulator pair per context
int crc32_on(Ctx& c, const void* d_data, uint64_t n_bytes, uint32_t* crc_out, hipStream_t s) {
    std::lock_guard<std::mutex> lk(c.crc.acc_mu);
    { const int rc = launch_crc(plan_crc(c, (const uint8_t*)d_data, n_bytes, c.crc.acc, nullptr, 0), s); if (rc) return rc; }
    uint32_t acc = 0;
    HIPCHK(hipMemcpyAsync(&acc, c.crc.acc, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    *crc_out = (crc_lead(n_bytes) ^ acc) ^ 0xFFFFFFFFu;               // the kernels leave the xor of the chunk remainders moved to the end of the stream
    return T3_OK;
}

// ---- N equal streams in one pass (t3_crc_frames.hip): stream f at d_data + f * stride, its results in slot f of the scratch ------------
// The scratch is cut into n_frames equal slots, and a slot is used the way the single-stream entry uses its whole scratch: the
// accumulator pair at its start, one (xor, sum) per CRC workgroup from kSlotPartialsOff on when there is room for them (then nothing
// is zeroed and nothing is added atomically).  All streams are equally long, so one decision serves them all, and every stream gets
// the W the single-stream plan gives one such stream: its partials are laid out as there.  One pass = at most one memset over the
// slots, one CRC launch over (workgroups per stream) x n_frames, one record launch.
constexpr uint64_t kSlotBytesMost = kSlotPartialsOff + 8ull * kRecordPartialWgs;   // a slot never uses more
uint64_t slot_bytes_of(uint64_t scratch_bytes, uint32_t n_frames) { return n_frames ? std::min<uint64_t>((scratch_bytes / n_frames) & ~15ull, kSlotBytesMost) : 0; }
struct CrcFramesPlan {
    bool one_pass;                                                   // false: the caller loops over the single-stream entry (one stream, T3HIP_CRC_BLOCKED, 2^40 bytes or more)
    CrcForm form;                                                    // Tables or Fp4Strided
    uint32_t n_frames, wgs_per_frame;                                // the CRC grid is (wgs_per_frame, n_frames); 0 workgroups: empty streams, no CRC launch
    uint32_t slot_bytes, n_partials;                                 // partials per stream; 0 = accumulators + atomics ...
    uint64_t zero_bytes;                                             // ... zeroed by one memset of this many bytes from the scratch's start
    CrcFramesArgs m; CrcChunksFramesArgs t;                          // crc_fp4_frames_kernel / crc_chunks_frames_kernel, by form
};
// slots: the wave slots the strided form spreads over (crc_slots); tab: the context's tables, or null for a plan that is only read.
// Fills arguments and grid; calls nothing in HIP.
CrcFramesPlan plan_crc_frames(uint32_t slots, const CrcTables* tab, const uint8_t* d_data, uint64_t n_bytes, uint64_t stride, uint32_t n_frames,
                              void* d_scratch, uint64_t scratch_bytes) {
    const CrcKnobs knob = crc_knobs();
    CrcFramesPlan p; memset(&p, 0, sizeof p);
    p.n_frames = n_frames; p.slot_bytes = (uint32_t)slot_bytes_of(scratch_bytes, n_frames);
    const bool in_limits = (n_bytes >> 11) < (1ull << 32) && n_bytes < (1ull << kCrcPows);
    p.one_pass = n_frames >= 2 && !knob.blocked && in_limits;
    uint32_t* acc = (uint32_t*)d_scratch;
    if (n_bytes >= 64 * 2048 && !knob.tables) {                       // (the entries hold base and stride to 16 bytes)
        CrcMArgs& m = p.m.m;
        m.data = d_data; m.n_bytes = n_bytes; m.n_rounds = (uint32_t)(n_bytes >> 11);
        m.tail_len = (uint32_t)(n_bytes - ((uint64_t)m.n_rounds << 11));
        int l = 0;                                                    // plan_crc's rule: halve W until a wave has at least 8 rounds
        while (l + 1 < kCrcStrideLevels && (uint64_t)crc_stride_w(slots, l) * 8 > m.n_rounds) ++l;
        m.stride_waves = crc_stride_w(slots, l); m.last_mod = (m.n_rounds - 1u) % m.stride_waves;
        if (tab) { m.afrag = tab->afrag4; m.zpow = tab->zpow; m.afb = tab->afb + (size_t)l * 64 * 4; m.dist_lo = tab->dist_lo; m.dist_hi = tab->dist_hi; }
        m.chunk_crc = acc; m.sym_sum = acc ? acc + 1 : nullptr;
        p.form = CrcForm::Fp4Strided; p.wgs_per_frame = m.stride_waves / 4 + (m.tail_len ? 1u : 0u);
        if (!knob.atomics && p.wgs_per_frame <= kRecordPartialWgs && p.slot_bytes >= kSlotPartialsOff + 8ull * p.wgs_per_frame) {
            m.partials = acc ? (uint32_t*)((uint8_t*)d_scratch + kSlotPartialsOff) : nullptr; p.n_partials = p.wgs_per_frame;
        }
        p.m.stride = stride; p.m.slot_bytes = p.slot_bytes; p.m.n_frames = n_frames;
    } else {
        CrcArgs& t = p.t.t;
        t.data = d_data; t.n_bytes = n_bytes; t.chunk_bytes = 2304;   // 256 words per lane
        t.n_chunks = (uint32_t)((n_bytes + t.chunk_bytes - 1) / t.chunk_bytes);
        t.chunk_crc = acc; t.sym_sum = acc ? acc + 1 : nullptr; t.zpow = tab ? tab->zpow : nullptr;
        p.form = CrcForm::Tables; p.wgs_per_frame = (t.n_chunks + 255) / 256;
        p.t.stride = stride; p.t.slot_bytes = p.slot_bytes; p.t.n_frames = n_frames;
    }
    p.zero_bytes = (p.n_partials || !n_frames) ? 0 : (uint64_t)(n_frames - 1) * p.slot_bytes + 8;
    return p;
}

// the pass of a plan with one_pass set: the CRC of every stream, then recs[f] for every f with frame_idx = first_idx + f * idx_step
int launch_crc_frames(const CrcFramesPlan& p, void* d_scratch, uint64_t n_words, uint64_t first_idx, uint64_t idx_step, uint32_t profile, uint32_t mode,
                      t3_frame_record* d_recs, hipStream_t s) {
    const bool fp4 = p.form == CrcForm::Fp4Strided;
    if (p.zero_bytes) HIPCHK(hipMemsetAsync(d_scratch, 0, p.zero_bytes, s));
    if (p.wgs_per_frame) {
        if (fp4) hipLaunchKernelGGL(crc_fp4_frames_kernel, dim3(p.wgs_per_frame, p.n_frames), dim3(256), 0, s, p.m);
        else hipLaunchKernelGGL(crc_chunks_frames_kernel, dim3(p.wgs_per_frame, p.n_frames), dim3(256), 0, s, p.t);
        HIPCHK(hipGetLastError());
    }
    RecordsArgs r; memset(&r, 0, sizeof r);
    r.scratch = (const uint8_t*)d_scratch; r.slot_bytes = p.slot_bytes; r.n_partials = p.n_partials;
    r.words = fp4 ? p.m.m.data : p.t.t.data; r.stride = fp4 ? p.m.stride : p.t.stride; r.n_words = n_words;
    r.first_idx = first_idx; r.idx_step = idx_step; r.lead = crc_lead(fp4 ? p.m.m.n_bytes : p.t.t.n_bytes); r.profile = profile; r.mode = mode; r.recs = d_recs;
    hipLaunchKernelGGL(frame_records_kernel, dim3(p.n_frames), dim3(64), 0, s, r);
    HIPCHK(hipGetLastError()); return T3_OK;
}

uint64_t r16(uint64_t x) { return (x + 15) & ~15ull; }
// what the batch entries hold their streams to (include/t3hip.h): at most 65535 of them, base and stride 16-byte aligned, the stride
// at least the stream's bytes rounded up to 16, no null base where there are bytes
bool frames_streams_ok(const void* d, uint64_t n_bytes, uint64_t stride, uint32_t n_frames) {
    return n_frames <= 65535 && (((uintptr_t)d | stride) & 15u) == 0 && stride >= r16(n_bytes) && (d || !n_bytes);
}

// CRC-32 of n_frames equal device streams on s, waited for: one pass into the context's scratch (slots, then one record per stream,
// which is where a stream's partials are folded), one copy back, one synchronise
int crc32_frames_on(Ctx& c, const uint8_t* d_data, uint64_t n_bytes, uint64_t stride, uint32_t n_frames, uint32_t* crc_out, hipStream_t s) {
    const uint64_t scr_bytes = kSlotBytesMost * n_frames;
    // a plan without addresses decides between the pass and the loop (which needs no scratch of this kind)
    if (!plan_crc_frames(crc_slots(c), nullptr, nullptr, n_bytes, stride, n_frames, nullptr, scr_bytes).one_pass) {
        for (uint32_t f = 0; f < n_frames; ++f) { const int rc = crc32_on(c, d_data + (uint64_t)f * stride, n_bytes, crc_out + f, s); if (rc) return rc; }
        return T3_OK;
    }
    std::lock_guard<std::mutex> lk(c.crc.acc_mu);
    void* scr; { const int rc = scratch(c, Scratch::StreamCrc, scr_bytes + sizeof(t3_frame_record) * (size_t)n_frames, &scr, s); if (rc) return rc; }
    t3_frame_record* d_recs = (t3_frame_record*)((uint8_t*)scr + scr_bytes);
    const CrcFramesPlan p = plan_crc_frames(crc_slots(c), &c.crc, d_data, n_bytes, stride, n_frames, scr, scr_bytes);
    { const int rc = launch_crc_frames(p, scr, n_bytes / 9, 0, 1, 0, 0, d_recs, s); if (rc) return rc; }
    std::vector<t3_frame_record> recs(n_frames);
    HIPCHK(hipMemcpyAsync(recs.data(), d_recs, sizeof(t3_frame_record) * (size_t)n_frames, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    for (uint32_t f = 0; f < n_frames; ++f) crc_out[f] = recs[f].crc32;
    return T3_OK;
}
}  // namespace

namespace t3 {
int crc_init(Ctx& c) {
    CrcTables& tab = c.crc;
    std::vector<uint32_t> z((size_t)kCrcPows * 32);                    // row j: the generator squared j times
    CrcOp sq = CrcOp::zero_byte();
    for (int j = 0; j < kCrcPows; ++j, sq = CrcOp::compose(sq, sq)) memcpy(&z[(size_t)j * 32], sq.col, sizeof sq.col);
    int rc = upload(tab.zpow, z); if (rc) return rc;
    HIPCHK(hipMalloc((void**)&tab.acc, 64));
    // FP4 slices.  8 data slices: column (step st, lane half kh, K slot pos) of the bit matrix = the remainder, at the end of a 64-byte
    // chunk, of the single input bit that K slot carries; rows = register bits.  In step st the lane's input dword w (bytes 4 st .. 4 st + 3
    // of its 32) is fed as the four dwords w & 0x11111111, w & 0x22222222, w & 0x44444444, (w >> 1) & 0x44444444 -- K slot pos = 8 j + p of
    // lane half kh carries bit 4 p + j of w, standing at nibble bit j (j < 3: FP4 0.5, 1.0, 2.0) or 2 (j = 3); the slice holds the
    // reciprocal weight, the product is 1.  Then the feedback slice of the blocked form (the running remainder 2048 bytes further on)
    // and five "append 64 * 2^b bytes" slices.
    std::vector<uint32_t> a4((size_t)14 * 64 * 4, 0u);
    static const uint32_t recip[4] = {4u, 2u, 1u, 1u};                 // weight nibble for a bit at nibble bit 0, 1, 2, 2
    CrcOp to_end[65]; to_end[0] = CrcOp::identity();                   // to_end[n]: append n zero bytes
    for (int n = 1; n <= 64; ++n) to_end[n] = CrcOp::compose(CrcOp::zero_byte(), to_end[n - 1]);
    for (int st = 0; st < 8; ++st) for (int kh = 0; kh < 2; ++kh) for (int pos = 0; pos < 32; ++pos) {
        const int j = pos >> 3, bit = 4 * (pos & 7) + j, o = 32 * kh + 4 * st + (bit >> 3);   // bit (bit & 7) of the chunk's byte o
        const uint32_t vec = to_end[64 - o].apply(1u << (bit & 7));
        for (int m = 0; m < 32; ++m) if (vec >> m & 1u) a4[((size_t)st * 64 + m + 32 * kh) * 4 + j] |= recip[j] << (4 * (pos & 7));
    }
    for (int st = 8; st < 14; ++st) remainder_slice(CrcOp::append_zero_bytes(st == 8 ? 2048u : 64u << (st - 9)), &a4[(size_t)st * 64 * 4]);
    rc = upload(tab.afrag4, a4); if (rc) return rc;
    std::vector<uint32_t> fb((size_t)kCrcStrideLevels * 64 * 4, 0u);   // feedback slices of the strided form, one per level
    for (int l = 0; l < kCrcStrideLevels; ++l) remainder_slice(CrcOp::append_zero_bytes(2048ull * crc_stride_w(crc_slots(c), l)), &fb[(size_t)l * 64 * 4]);
    rc = upload(tab.afb, fb); if (rc) return rc;
    // A strided wave's distance to the stream's end, tail_len + 2048 hi bytes (hi < its W <= W0), by table instead of bit by bit:
    // "append n bytes", n < 2048, and "append 2048 n bytes", n <= W0, by repeated composition; entry 0 of both is the identity
    const uint32_t w0 = crc_stride_w(crc_slots(c), 0);
    std::vector<uint32_t> lo((size_t)2048 * 32), hi(((size_t)w0 + 1) * 32);
    const CrcOp one = CrcOp::zero_byte(), round = CrcOp::append_zero_bytes(2048);
    CrcOp op = CrcOp::identity();
    for (uint32_t n = 0; n < 2048; ++n, op = CrcOp::compose(one, op)) memcpy(&lo[(size_t)n * 32], op.col, sizeof op.col);
    op = CrcOp::identity();
    for (uint32_t n = 0; n <= w0; ++n, op = CrcOp::compose(round, op)) memcpy(&hi[(size_t)n * 32], op.col, sizeof op.col);
    rc = upload(tab.dist_lo, lo); if (rc) return rc;
    return upload(tab.dist_hi, hi);
}
}  // namespace t3

extern "C" {

uint64_t t3hip_frame_record_scratch_bytes(uint64_t) { return 64 + 8ull * kRecordPartialWgs; }   // two accumulators | one (xor, sum) per CRC workgroup; 64 bytes still work (accumulators + atomics)
int t3hip_frame_record_dev(const void* d_words, uint64_t n_words, uint64_t frame_idx, const t3_cfg* cfg, t3_frame_record* d_rec,
                           void* d_scratch, uint64_t scratch_bytes, void* stream) {
    Ctx& c = ctx(); if (!c.ready) return T3_E_NODEVICE;
    if (!cfg || !d_rec || (n_words && !d_words) || !d_scratch || scratch_bytes < 8) return T3_E_ARG;
    hipStream_t s = (hipStream_t)stream;
    const uint64_t n_bytes = 9 * n_words;
    uint32_t* parts = scratch_bytes >= 64 + 8 ? (uint32_t*)((uint8_t*)d_scratch + 64) : nullptr;
    const uint32_t cap_wg = parts ? (uint32_t)std::min<uint64_t>((scratch_bytes - 64) / 8, kRecordPartialWgs) : 0u;
    const CrcPlan p = plan_crc(c, (const uint8_t*)d_words, n_bytes, (uint32_t*)d_scratch, parts, cap_wg);
    { const int rc = launch_crc(p, s); if (rc) return rc; }
    hipLaunchKernelGGL(frame_record_kernel, dim3(1), dim3(64), 0, s, (const uint32_t*)d_scratch, crc_lead(n_bytes), (const uint8_t*)d_words, n_words, frame_idx, (uint32_t)cfg->profile, (uint32_t)cfg->mode, (void*)d_rec, (const uint32_t*)parts, p.n_partials);
    HIPCHK(hipGetLastError()); return T3_OK;
}

int t3hip_crc32_dev(const void* d_data, uint64_t n_bytes, uint32_t* crc_out, void* stream) {
    Ctx& c = ctx(); if (!c.ready) return T3_E_NODEVICE;
    if (!crc_out || (n_bytes && !d_data)) return T3_E_ARG;
    return crc32_on(c, d_data, n_bytes, crc_out, (hipStream_t)stream);
}

int t3hip_crc32(const void* data, uint64_t n_bytes, uint32_t* crc_out) {
    Ctx& c = ctx(); if (!c.ready) return T3_E_NODEVICE;
    if (!crc_out || (n_bytes && !data)) return T3_E_ARG;
    std::lock_guard<std::recursive_mutex> hl(c.host_mu);
    void* di; int rc = scratch(c, Scratch::HostIn, n_bytes + 64, &di); if (rc) return rc;
    if (n_bytes) HIPCHK(hipMemcpyAsync(di, data, n_bytes, hipMemcpyHostToDevice, c.stream));
    return crc32_on(c, di, n_bytes, crc_out, c.stream);
}

// ---- N equal frames: records and payload CRCs in one pass (argument checks first, then the device: the batch rule of t3hip.h) ----
uint64_t t3hip_frame_records_scratch_bytes(uint64_t n_words, uint32_t n_frames) { return t3hip_frame_record_scratch_bytes(n_words) * n_frames; }

int t3hip_frame_records_plan(uint64_t n_words, uint32_t n_frames, uint32_t n_cu, uint64_t scratch_bytes, t3_records_plan* out) {
    if (!out || n_frames > 65535 || n_words >= (1ull << 60) || scratch_bytes < 16ull * n_frames) return T3_E_ARG;
    uint32_t slots = n_cu * 8u;                                       // crc_slots of a part with n_cu CUs
    if (!n_cu) { Ctx& c = ctx(); if (!c.ready) return T3_E_NODEVICE; slots = crc_slots(c); }
    const uint64_t n_bytes = 9 * n_words;
    const CrcFramesPlan p = plan_crc_frames(slots, nullptr, nullptr, n_bytes, r16(n_bytes), n_frames, nullptr, scratch_bytes);
    memset(out, 0, sizeof *out);
    out->n_frames = n_frames; out->one_pass = p.one_pass ? 1 : 0; out->form = p.form == CrcForm::Fp4Strided ? T3_RECORDS_FP4 : T3_RECORDS_TABLES;
    out->stride_waves = p.m.m.stride_waves; out->wgs_per_frame = p.wgs_per_frame; out->partials_per_frame = p.n_partials;
    out->frame_bytes = n_bytes; out->stride_min = r16(n_bytes); out->scratch_bytes = (uint64_t)p.slot_bytes * n_frames;
    return T3_OK;
}

int t3hip_frame_records_dev(const void* d_words, uint64_t n_words, uint64_t stride, uint32_t n_frames, uint64_t first_idx, uint64_t idx_step,
                            const t3_cfg* cfg, t3_frame_record* d_recs, void* d_scratch, uint64_t scratch_bytes, void* stream) {
    if (!cfg || n_words >= (1ull << 60) || !frames_streams_ok(d_words, 9 * n_words, stride, n_frames)) return T3_E_ARG;
    if (n_frames && (!d_recs || !d_scratch || ((uintptr_t)d_scratch & 15u) || scratch_bytes < 16ull * n_frames)) return T3_E_ARG;
    Ctx& c = ctx(); if (!c.ready) return T3_E_NODEVICE;
    if (!n_frames) return T3_OK;
    const CrcFramesPlan p = plan_crc_frames(crc_slots(c), &c.crc, (const uint8_t*)d_words, 9 * n_words, stride, n_frames, d_scratch, scratch_bytes);
    if (p.one_pass) return launch_crc_frames(p, d_scratch, n_words, first_idx, idx_step, (uint32_t)cfg->profile, (uint32_t)cfg->mode, d_recs, (hipStream_t)stream);
    for (uint32_t f = 0; f < n_frames; ++f) {                        // the single-frame entry on frame f and slot f: the same bytes
        const int rc = t3hip_frame_record_dev((const uint8_t*)d_words + (uint64_t)f * stride, n_words, first_idx + (uint64_t)f * idx_step, cfg, d_recs + f,
                                              (uint8_t*)d_scratch + (uint64_t)f * p.slot_bytes, p.slot_bytes, stream);
        if (rc) return rc;
    }
    return T3_OK;
}

int t3hip_crc32_frames_dev(const void* d_data, uint64_t n_bytes, uint64_t stride, uint32_t n_frames, uint32_t* crc_out, void* stream) {
    if ((n_frames && !crc_out) || !frames_streams_ok(d_data, n_bytes, stride, n_frames)) return T3_E_ARG;
    Ctx& c = ctx(); if (!c.ready) return T3_E_NODEVICE;
    if (!n_frames) return T3_OK;
    if (!n_bytes) { memset(crc_out, 0, 4 * (size_t)n_frames); return T3_OK; }   // what the containers store for an empty payload
    return crc32_frames_on(c, (const uint8_t*)d_data, n_bytes, stride, n_frames, crc_out, (hipStream_t)stream);
}

int t3hip_crc32_frames(const void* const* frames, uint64_t n_bytes, uint32_t n_frames, uint32_t* crc_out) {
    if (n_frames > 65535 || (n_frames && (!crc_out || !frames))) return T3_E_ARG;
    for (uint32_t f = 0; f < n_frames && n_bytes; ++f) if (!frames[f]) return T3_E_ARG;
    Ctx& c = ctx(); if (!c.ready) return T3_E_NODEVICE;
    if (!n_frames) return T3_OK;
    if (!n_bytes) { memset(crc_out, 0, 4 * (size_t)n_frames); return T3_OK; }
    std::lock_guard<std::recursive_mutex> hl(c.host_mu);
    const uint64_t stride = r16(n_bytes);
    void* di; { const int rc = scratch(c, Scratch::HostIn, stride * n_frames + 64, &di); if (rc) return rc; }
    for (uint32_t f = 0; f < n_frames; ++f) HIPCHK(hipMemcpyAsync((uint8_t*)di + (uint64_t)f * stride, frames[f], n_bytes, hipMemcpyHostToDevice, c.stream));
    return crc32_frames_on(c, (const uint8_t*)di, n_bytes, stride, n_frames, crc_out, c.stream);
}

int t3hip_index_assemble(t3_frame_record* recs, uint64_t n, uint64_t first_payload_offset) {
    if (n && !recs) return T3_E_ARG;
    std::sort(recs, recs + n, [](const t3_frame_record& x, const t3_frame_record& y) { return x.frame_idx < y.frame_idx; });
    uint64_t off = first_payload_offset;
    for (uint64_t i = 0; i < n; ++i) { recs[i].byte_offset = off; off += 9 * recs[i].n_words; }
    return T3_OK;
}

}  // extern "C"
